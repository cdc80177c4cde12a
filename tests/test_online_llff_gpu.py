"""GPU: online distillation on an LLFF scene (r2l_llff_rand_poses in csrc/r2l_online.hip, online.LLFFOnlineTeacherSource, the
--kd_online branch of train.train with --dataset_type llff).

The pose kernel against the float64 numpy mirror of tests/test_online_llff_cpu.py, bit for bit; the source against the mirror of
r2l_rand_rays fed the kernel's poses, the engine it wraps (bit for bit) and the CPU oracle's NDC teacher at the base focal (the 1e-4
rgb contract); the loop through frontend.main against a hand-written loop over source.batch -> R2LTrainer.step, against itself, and
across --resume, bit for bit.  The scene is tests/golden/llff/scene: 10 views of 30 x 40, focal 37.5, views {0, 8} held out."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O
from test_online_cpu import host_rays
from test_online_llff_cpu import CORNERS, SCENE, mirror_poses

pytestmark = pytest.mark.gpu
H, W, FOCAL = 30, 40, 37.5
LLFF = ['--dataset_type', 'llff', '--factor', '8', '--llffhold', '8', '--datadir', SCENE]
TEACHER_NET = ['--model_name', 'nerf', '--use_viewdirs', '--N_importance', '128']
CHUNK = 100


@pytest.fixture(scope='module')
def state(pkg, built_lib):
    from efficient_nerf_amd import llff
    return llff.load_scene(SCENE).rand_state


@pytest.fixture(scope='module')
def teacher():
    return O.make_teacher_state(1), O.make_teacher_state(2)


# ---- 1. r2l_llff_rand_poses ------------------------------------------------------------------------------------------------------
def _launch(u, box, focal):
    from efficient_nerf_amd._lib import check, current_stream, dptr, lib
    n, n_u = u.shape
    ud = torch.from_numpy(np.ascontiguousarray(u)).cuda()
    po = torch.full((n + 1, 3, 4), -7., dtype=torch.float32, device='cuda')       # a guard row behind the last pose and the last focal
    fo = torch.full((n + 1,), -7., dtype=torch.float32, device='cuda')
    check(lib().r2l_llff_rand_poses(C.c_void_p(ud.data_ptr()), n, n_u, box.ctypes.data_as(C.c_void_p), focal, dptr(po), dptr(fo), current_stream()))
    torch.cuda.synchronize()
    assert (po[n] == -7).all() and fo[n] == -7                                    # nothing written behind row n - 1
    return po[:n].cpu().numpy(), fo[:n].cpu().numpy()


@pytest.mark.parametrize('n_pose', [1, 63, 64, 65, 257])
def test_rand_poses_bit_for_bit(state, n_pose):
    """the wave edge and the block tail, with and without the focal draw: poses and focals are the mirror's"""
    from efficient_nerf_amd import llff
    box = llff.pose_box(state)
    u7 = np.random.RandomState(n_pose).rand(n_pose, 7)
    u7[:2, :6] = np.array(CORNERS)[:n_pose]               # the probe corners of `--precision auto` are among the inputs
    for n_u in (7, 6):
        u = np.ascontiguousarray(u7[:, :n_u])
        poses, focals = _launch(u, box, FOCAL)
        want_p, want_f = mirror_poses(box, u, FOCAL)
        assert poses.dtype == want_p.dtype == np.float32 and poses.tobytes() == want_p.tobytes()
        assert focals.tobytes() == want_f.tobytes()
        assert np.array_equal(focals, (FOCAL * (u[:, 6] + 1)).astype(np.float32) if n_u == 7 else np.full(n_pose, np.float32(FOCAL)))
        again = _launch(u, box, FOCAL)
        assert again[0].tobytes() == poses.tobytes() and again[1].tobytes() == focals.tobytes()      # the same arguments, the same bytes
        R = poses[:, :, :3].astype(np.float64)            # a sanity line, not a tolerance: each rotation is orthonormal
        assert np.abs(np.einsum('nij,nik->njk', R, R) - np.eye(3)).max() < 1e-6
        for row, pose in zip(CORNERS[:n_pose], poses):    # ... and the corners are the host path's corners to two float32 ulps
            assert np.abs(pose - llff.pose_in_boxes(state, row[:3], row[3:])[:3, :4]).max() <= 2. ** -22


# ---- 2. LLFFOnlineTeacherSource ------------------------------------------------------------------------------------------------------
def ndc_teacher(teacher, rays_o, rays_d, focal):
    """the reference's render(..., ndc=True) of given world-space rays: view directions first, then ndc_rays(H, W, focal, 1., ...) and
    the two passes over [0, 1] (main.py:148-162, 624-756); as tests/test_llff_gpu.py states it"""
    vd = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
    o, d = O.ndc_rays(H, W, focal, 1., rays_o, rays_d)
    with torch.no_grad():
        return torch.cat([O.render_rays(teacher[0], teacher[1], o[s:s + CHUNK], d[s:s + CHUNK], near=0., far=1., white_bkgd=False,
                                        viewdirs=vd[s:s + CHUNK])['rgb_map'] for s in range(0, o.shape[0], CHUNK)], 0)


def test_source_targets_are_the_ndc_teachers(state, teacher):
    from efficient_nerf_amd import create_data as CDm
    from efficient_nerf_amd import frontend as fe
    from efficient_nerf_amd import llff
    from efficient_nerf_amd.online import LLFFOnlineTeacherSource
    seed, n_pose, n, t = 3, 3, 300, 4
    eng = CDm.build_llff_teacher_engine(fe.parse_args(TEACHER_NET + LLFF + ['--precision', 'fp16x3']),
                                        {'network_fn_state_dict': teacher[0], 'network_fine_state_dict': teacher[1]}, (H, W, FOCAL), state)
    assert eng.ndc and eng.precision_name == 'fp16x3'
    lines = []
    src = LLFFOnlineTeacherSource(eng, H, W, FOCAL, state, n_pose=n_pose, seed=seed, watch_every=2, log=lines.append)
    ro, rd, target = src.batch(t, n)                                             # a watched step
    assert all(x.shape == (n, 3) and x.is_cuda and x.dtype == torch.float32 for x in (ro, rd, target)) and not lines and not src.fallbacks
    # the poses: the mirror's, from this step's uniform draws; the rays: r2l_rand_rays' mirror fed the kernel's poses and focals read back
    u = np.random.RandomState((seed, t)).rand(n_pose, 7)
    assert np.array_equal(src.uniforms(t), u)
    poses, focals = src.draws(t)
    want_p, want_f = mirror_poses(llff.pose_box(state), u, FOCAL)
    assert poses.numpy().tobytes() == want_p.tobytes() and focals.dtype == np.float64 and np.array_equal(focals, want_f.astype(np.float64))
    assert ((focals >= FOCAL) & (focals < 2 * FOCAL)).all()
    mo, md, _ = host_rays(poses.numpy(), focals.astype(np.float32), H, W, seed, t, n)
    assert np.array_equal(ro.cpu().numpy(), mo) and np.array_equal(rd.cpu().numpy(), md)
    # the target: the engine's render of those rays bit for bit, and the oracle's NDC teacher at the BASE focal within the rgb contract
    keep = [x.clone() for x in (ro, rd, target)]
    assert torch.equal(target, eng.render_rays(ro, rd)['rgb_map'])
    diff = (target.cpu() - ndc_teacher(teacher, ro.cpu(), rd.cpu(), FOCAL)).abs().max().item()
    print(f'online LLFF target vs the CPU oracle\'s NDC teacher at the base focal on {n} rays: L_inf {diff:.3e} ({eng.precision_name})')
    assert diff <= 1e-4
    # a batch is a function of (seed, step): step t + 1 differs, and step t comes back after it
    nxt = src.batch(t + 1, n)
    assert not torch.equal(nxt[1], keep[1])
    assert all(torch.equal(a, b) for a, b in zip(src.batch(t, n), keep))
    fixed = LLFFOnlineTeacherSource(eng, H, W, FOCAL, state, n_pose=n_pose, seed=seed, use_rand_focal=False, watch_every=0)
    fo, fd, _ = fixed.batch(t, 64)
    p6, f6 = mirror_poses(llff.pose_box(state), np.random.RandomState((seed, t)).rand(n_pose, 6), FOCAL)
    mo, md, _ = host_rays(p6, f6, H, W, seed, t, 64)
    assert f6.tolist() == [FOCAL] * n_pose and np.array_equal(fo.cpu().numpy(), mo) and np.array_equal(fd.cpu().numpy(), md)
    eng.close()


# ---- 3. the loop -----------------------------------------------------------------------------------------------------------------
NET = ['--model_name', 'R2L', '--netdepth', '6', '--netwidth', '32', '--n_sample_per_ray', '4', '--multires', '4', '--use_residual', '--trial.ON',
       '--trial.body_arch', 'resmlp'] + LLFF
SPLIT, N_RAND = 256, 2


@pytest.fixture(scope='module')
def setup(pkg, built_lib, teacher, tmp_path_factory):
    """a synthetic 8 x 256 teacher's checkpoint and its flags as a config file, the student's first weights as a checkpoint (no run
    draws its own)"""
    from efficient_nerf_amd import frontend as fe, train as T
    root = tmp_path_factory.mktemp('online_llff')
    ck, cfg = str(root / 'teacher.tar'), root / 'teacher.txt'
    fe.save_checkpoint(ck, *teacher)
    cfg.write_text('dataset_type = llff\nuse_viewdirs = True\nN_samples = 64\nN_importance = 128\n')
    s = {'root': str(root), 'teacher': ck, 'config': str(cfg), 'init': str(root / 'init.tar')}
    tr = T.trainer_from_args(fe.parse_args(_argv(s, 'x')), 8)
    fe.save_checkpoint(s['init'], T.init_state_dict(tr.plan, seed=7))
    return s


def _argv(s, expname, n_iters=4, extra=()):
    return NET + ['--kd_online', '--teacher_ckpt', s['teacher'], '--teacher_config', s['config'], '--N_rand', str(N_RAND), '--kd_online_split',
                  str(SPLIT), '--kd_online_poses', '3', '--kd_online_seed', '4', '--kd_online_watch', '2', '--N_iters', str(n_iters), '--perturb', '0',
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
    """the uninterrupted four-step run through frontend.main's train, once for the tests that compare with it: (its log lines, its
    ckpt.tar)"""
    from efficient_nerf_amd import frontend as fe, train as T
    lines = []
    T.train(fe.parse_args(_argv(setup, 'whole')), log=lines.append)
    return lines, torch.load(os.path.join(setup['root'], 'whole', 'weights', 'ckpt.tar'), map_location='cpu', weights_only=False)


def test_loop_start_up_train_and_test_lines(setup, whole):
    lines, ck = whole
    start = [ln for ln in lines if ln.startswith('Online distillation')]
    assert len(start) == 1 and '\n' not in start[0]
    for part in (f'teacher "{setup["teacher"]}" in fp16x3', '3 random poses of 30 x 40 per step', 'focal 37.50 .. 75.00', f'pose boxes of "{SCENE}"',
                 'seed 4', 'watched every 2 steps', f'{N_RAND * SPLIT} rays per step + 0 hard rays'):
        assert part in start[0], (part, start[0])
    assert not any(ln.startswith('Found ') for ln in lines)
    train = [re.match(r'^\[TRAIN\] Iter (\d+) data_time (\S+) batch_time (\S+) loss (\S+) psnr (\S+) hist_psnr (\S+) LR (\d\.\d{10})$', ln)
             for ln in lines if ln.startswith('[TRAIN]')]
    assert len(train) == 4 and all(train) and [int(m.group(1)) for m in train] == [1, 2, 3, 4]
    assert all(np.isfinite(float(m.group(4))) for m in train)
    # the held-out views {0, 8} of the scene, rendered at iterations 2 and 4
    assert any(ln.startswith('Test split: 2 view(s) 30 x 40') for ln in lines)
    tests = [ln for ln in lines if ln.startswith('[TEST] Iter')]
    assert len(tests) == 2 and tests[0].startswith('[TEST] Iter 2 TestPSNR ') and tests[1].startswith('[TEST] Iter 4 TestPSNR '), tests
    assert ck['global_step'] == 4


def test_loop_is_source_batch_then_trainer_step(setup, whole):
    """weights and Adam moments after four steps of the command line = a hand-written loop over source.batch(i) -> R2LTrainer.step"""
    from efficient_nerf_amd import frontend as fe, online, train as T
    args = fe.parse_args(_argv(setup, 'hand'))
    tr = T.trainer_from_args(args, N_RAND * SPLIT)
    tr.load_state_dict(fe.load_checkpoint(setup['init'])['network_fn_state_dict'])
    src, _ = online.source_from_args(args, log=lambda *a: None)
    assert isinstance(src, online.LLFFOnlineTeacherSource) and (src.H, src.W, src.focal) == (H, W, FOCAL) and src.engine.ndc
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
    from efficient_nerf_amd import frontend as fe
    lines, again = _main(setup, 'again', capsys)
    assert _same_state(whole[1], again) and sum(ln.startswith('[TRAIN] Iter') for ln in lines) == 4
    _, first = _main(setup, 'first', capsys, n_iters=2)
    assert first['global_step'] == 2 and not _same_state(whole[1], first)
    argv = _argv(setup, 'resumed')
    argv[argv.index('--pretrained_ckpt') + 1] = os.path.join(setup['root'], 'first', 'weights', 'ckpt.tar')
    capsys.readouterr()
    assert fe.main(argv + ['--resume']) == 0
    out = capsys.readouterr().out.splitlines()
    assert 'Resume optimizer successfully.' in out and [ln.split()[2] for ln in out if ln.startswith('[TRAIN] Iter')] == ['3', '4']
    resumed = torch.load(os.path.join(setup['root'], 'resumed', 'weights', 'ckpt.tar'), map_location='cpu', weights_only=False)
    assert resumed['global_step'] == 4 and _same_state(whole[1], resumed)
