#!/usr/bin/env python
"""What online distillation (train.py --kd_online, efficient-nerf_amd/online.py) costs per step at the README batch: 81,920 fresh rays of
100 random 400 x 400 poses rendered by the teacher + 16,384 rows from the hard-ray pool = 98,304 rays through a W256D88 student.

Timed with HIP events, in windows of --steps repetitions, --repeat windows per quantity after --warmup untimed repetitions; a line
gives the median window and the spread (smallest .. largest window), per repetition:
  r2l_rand_rays          the ray launch alone
  spot check             NeRFEngine.spot_check of one batch (every --kd_online_watch-th step runs one)
  teacher render         engine.render_rays on the batch's rays, in the mode `--precision auto` picks for create_data rand
                         (choose_precision_for_rand), for a synthetic teacher and for tests/golden/trained_like's
  student step           R2LTrainer.step at 98,304 rays: the shard path's step (tools/train_time.py's launches and shapes; the
                         figure of profiles/train_step_time.txt is quoted beside it)
  online step            source.batch + the pool rows + R2LTrainer.step, as train() runs them, the host's draws included
and the ratio online step / student step.  Writes profiles/train_online_time.txt.

--llff: the same on an LLFF scene (online.LLFFOnlineTeacherSource): the pose state of tests/golden/llff/scene at fern's size, 378 x 504
at focal 407, the NDC teacher (near, far = 0, 1) in the mode `--precision auto` picks on llff_probe_rays, the student at near, far =
0, 1.  Its lines, side by side:
  r2l_llff_rand_poses    the pose kernel with the upload of the step's 100 x 7 uniform draws
  r2l_rand_rays          the ray launch alone, on the poses the kernel left on the device
  teacher render         the NDC engine's render_rays on the batch's rays
  student step, online step and their ratio, as above
  host pose loop         the wall time of what the pose kernel replaces, 100 x (LLFFRandStream.rand_pose + the focal draw), on this
                         machine's host, beside the one RandomState.rand call that is left
Writes profiles/train_online_llff_time.txt.

    python tools/train_online_time.py [--llff] [--steps 10] [--repeat 5] [--warmup 3] [--out profiles/train_online_time.txt]
"""
import argparse
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import _pkg  # noqa: E402

_pkg.load()
from efficient_nerf_amd import NeRFEngine, PRECISIONS  # noqa: E402
from efficient_nerf_amd.create_data import choose_precision_for_rand  # noqa: E402
from efficient_nerf_amd.online import OnlineTeacherSource  # noqa: E402
from efficient_nerf_amd.train import R2LTrainer, init_state_dict  # noqa: E402
from oracle import r2l_oracle as O  # noqa: E402

N_ONLINE, N_POOL, N_POSE, HW = 81920, 16384, 100, 400


def windows(fn, steps, repeat, warmup):
    """per-repetition ms of `repeat` windows of `steps` calls each (HIP events), and the host's wall clock likewise"""
    for _ in range(warmup):
        fn()
    dev, wall = [], []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / steps)
        dev.append(a.elapsed_time(b) / steps)
    return dev, wall


def fmt(ms, unit='ms', scale=1.):
    return f'{statistics.median(ms) * scale:.2f} {unit} ({min(ms) * scale:.2f} .. {max(ms) * scale:.2f})'


LLFF_H, LLFF_W, LLFF_FOCAL = 378, 504, 407.


def write(lines, out):
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, 'w') as f:
        f.write(text)


def main_llff(a):
    from efficient_nerf_amd import frontend as fe, llff
    from efficient_nerf_amd.create_data import LLFFRandStream, build_llff_teacher_engine
    from efficient_nerf_amd.online import LLFFOnlineTeacherSource
    H, W, focal = LLFF_H, LLFF_W, LLFF_FOCAL
    n = N_ONLINE + N_POOL
    scene_dir = os.path.join(ROOT, 'tests', 'golden', 'llff', 'scene')
    state = llff.load_scene(scene_dir).rand_state
    targs = fe.parse_args(['--model_name', 'nerf', '--use_viewdirs', '--N_samples', '64', '--N_importance', '128', '--dataset_type', 'llff',
                           '--datadir', scene_dir, '--precision', 'auto'])
    auto = []
    eng = build_llff_teacher_engine(targs, {'network_fn_state_dict': O.make_teacher_state(1), 'network_fine_state_dict': O.make_teacher_state(2)},
                                    (H, W, focal), state, log=auto.append)
    src = LLFFOnlineTeacherSource(eng, H, W, focal, state, n_pose=N_POSE, seed=0, watch_every=100, log=lambda *x: None)
    tr = R2LTrainer(0., 1., netdepth=88, netwidth=256, use_residual=True, trial=dict(body_arch='resmlp'), max_rays=n)
    tr.load_state_dict(init_state_dict(tr.plan, seed=0))
    g = torch.Generator().manual_seed(0)
    t_rand = torch.rand(n, 16, generator=g).cuda()
    ro, rd, tgt = (x.clone() for x in src.batch(1, n))                       # the student's own batch: rays of the scene, the teacher's colours
    pool = torch.cat([ro[:N_POOL], rd[:N_POOL], tgt[:N_POOL]], -1)
    student = lambda: tr.step(ro, rd, tgt, 1e-4, 1., t_rand)[0].item()          # with the loop's read of the loss
    lines = [f'Online distillation on an LLFF scene at the README batch: {N_ONLINE} rays of {N_POSE} random {H} x {W} poses (focal {focal:g} x [1, 2), '
             f'the pose boxes of tests/golden/llff/scene) per step from the NDC teacher + {N_POOL} hard-ray rows = {n} rays, W256D88 student '
             f'({tr.n_param} parameters) at near, far = 0, 1; HIP events, median of {a.repeat} windows of {a.steps} repetitions after {a.warmup} '
             f'warm-up repetitions (smallest .. largest window)',
             f'synthetic teacher (oracle.make_teacher_state(1), (2)), 64 + 128 samples, mode chosen by auto: {eng.precision_name} (probe differences '
             f'{eng.auto_diffs})']
    st_dev, _ = windows(student, a.steps, a.repeat, a.warmup)
    pose_dev, pose_wall = windows(lambda: src.poses(1), 20 * a.steps, a.repeat, a.warmup)
    po, fo = src.poses(1)
    rays, _ = windows(lambda: src._launch_rays(po, fo, 1, N_ONLINE), 20 * a.steps, a.repeat, a.warmup)
    o1, d1 = src._launch_rays(po, fo, 1, N_ONLINE)
    render, _ = windows(lambda: eng.render_rays(o1, d1), a.steps, a.repeat, a.warmup)
    step = [1]

    def online():
        step[0] += 1
        bo, bd, bt = src.batch(step[0], N_ONLINE)
        bo, bd, bt = (torch.cat([x, pool[:, 3 * k:3 * k + 3]], 0) for k, x in enumerate((bo, bd, bt)))
        torch.cuda.synchronize()                                          # the loop's data_time bracket
        tr.step(bo, bd, bt, 1e-4, 1., t_rand)[0].item()

    def host_loop(k):                       # what create_data rand runs per save group, and what the kernel replaces per step
        stream = LLFFRandStream(state, seed=(0, k))
        t0 = time.perf_counter()
        for _ in range(N_POSE):
            stream.rand_pose()
            focal * stream.rand_focal_scale()
        return (time.perf_counter() - t0) * 1e3

    def host_rand(k):
        t0 = time.perf_counter()
        src.uniforms(k)
        return (time.perf_counter() - t0) * 1e3
    host_loop(0)
    loop_ms = [host_loop(k) for k in range(1, a.repeat + 1)]
    rand_ms = [host_rand(k) for k in range(1, a.repeat + 1)]
    on_dev, on_wall = windows(online, a.steps, a.repeat, a.warmup)
    st2, _ = windows(student, a.steps, a.repeat, 1)                        # the student step again, beside the online windows
    ratio = statistics.median(on_wall) / statistics.median(st2)
    lines += [f'  r2l_llff_rand_poses, {N_POSE} poses (incl. RandomState((seed, step)).rand({N_POSE}, 7) and its upload, {N_POSE * 7 * 8} bytes): '
              f'{fmt(pose_dev, "us", 1e3)} on the device, {fmt(pose_wall, "us", 1e3)} on the host\'s clock',
              f'  r2l_rand_rays, {N_ONLINE} rays of those poses (already on the device): {fmt(rays, "us", 1e3)}',
              f'  teacher render of those rays (NDC render_rays, {eng.precision_name}): {fmt(render)} = {N_ONLINE / statistics.median(render) * 1e3:.3e} rays/s',
              f'  student step (R2LTrainer.step, {n} rays): {fmt(st_dev)}; beside the online windows: {fmt(st2)}',
              f'  online step (source.batch + pool rows + R2LTrainer.step; {src.checks} spot check(s), {len(src.fallbacks)} fallback(s) in '
              f'{step[0] - 1} steps): {fmt(on_dev)} on the device, {fmt(on_wall)} on the host\'s clock',
              f'  online step / shard step = {ratio:.3f} (host clock of the online step over the student step; render + rays + poses alone would '
              f'add {(statistics.median(render) + statistics.median(rays) + statistics.median(pose_dev)) / statistics.median(st2):.3f})',
              f'  host pose loop the kernel replaces ({N_POSE} x LLFFRandStream.rand_pose + focal, numpy {np.__version__}, wall clock of this '
              f'machine\'s host, {a.repeat} runs): {fmt(loop_ms)} = {statistics.median(loop_ms) * 1e3 / N_POSE:.0f} us a pose; the one rand call left '
              f'on the host: {fmt(rand_ms, "us", 1e3)}']
    eng.close()
    write(lines, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--llff', action='store_true')
    ap.add_argument('--out', type=str, default='')
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', 'train_online_llff_time.txt' if a.llff else 'train_online_time.txt')
    if not torch.cuda.is_available():
        raise SystemExit('tools/train_online_time.py measures on the device: no HIP device is visible')
    if a.llff:
        return main_llff(a)
    n = N_ONLINE + N_POOL
    focal = O.focal_from_angle(HW)
    tr = R2LTrainer(netdepth=88, netwidth=256, use_residual=True, trial=dict(body_arch='resmlp'), max_rays=n)
    tr.load_state_dict(init_state_dict(tr.plan, seed=0))
    g = torch.Generator().manual_seed(0)
    # the student step of tools/train_time.py: the same launches on the same shapes
    ro = (torch.tensor([0., 0., 4.]) + 0.2 * torch.randn(n, 3, generator=g)).cuda()
    rd = torch.nn.functional.normalize(-ro.cpu() + 0.8 * torch.randn(n, 3, generator=g), dim=-1).cuda()
    tgt = torch.rand(n, 3, generator=g).cuda()
    t_rand = torch.rand(n, 16, generator=g).cuda()
    pool = torch.cat([ro[:N_POOL], rd[:N_POOL], tgt[:N_POOL]], -1)
    student = lambda: tr.step(ro, rd, tgt, 1e-4, 1., t_rand)[0].item()          # with the loop's read of the loss
    lines = [f'Online distillation at the README batch: {N_ONLINE} rays of {N_POSE} random {HW} x {HW} poses per step from the teacher + {N_POOL} '
             f'hard-ray rows = {n} rays, W256D88 student ({tr.n_param} parameters); HIP events, median of {a.repeat} windows of {a.steps} '
             f'repetitions after {a.warmup} warm-up repetitions (smallest .. largest window)']
    st_dev, _ = windows(student, a.steps, a.repeat, a.warmup)
    parent = None
    try:
        with open(os.path.join(ROOT, 'profiles', 'train_step_time.txt')) as f:
            parent = float(re.search(r'^step: (\S+) ms', f.read(), re.M).group(1))
    except (OSError, AttributeError):
        pass
    lines.append(f'student step (R2LTrainer.step, {n} rays, the shard path\'s step without its reads from the disk): {fmt(st_dev)}' +
                 (f'; profiles/train_step_time.txt: {parent:.2f} ms (one window of 5 steps), this run / that = {statistics.median(st_dev) / parent:.3f}'
                  if parent else ''))
    tl = os.path.join(ROOT, 'tests', 'golden', 'trained_like')
    npz = lambda name: {k: torch.from_numpy(v) for k, v in np.load(os.path.join(tl, name)).items()}
    teachers = [('synthetic teacher (oracle.make_teacher_state(1), (2))', lambda: (O.make_teacher_state(1), O.make_teacher_state(2))),
                ('tests/golden/trained_like\'s teacher', lambda: (npz('teacher_coarse.npz'), npz('teacher_fine.npz')))]
    for name, make in teachers:
        eng = NeRFEngine(HW, HW, focal, precision=PRECISIONS['fp16x3']).load_state_dicts(*make())
        mode = choose_precision_for_rand(eng, HW, HW, focal)
        src = OnlineTeacherSource(eng, HW, HW, focal, n_pose=N_POSE, seed=0, watch_every=100, log=lambda *x: None)
        step = [0]
        poses, focals = src.draws(1)
        f32 = torch.from_numpy(focals).to(torch.float32)
        rays, _ = windows(lambda: src._launch_rays(poses, f32, 1, N_ONLINE), 20 * a.steps, a.repeat, a.warmup)
        o1, d1 = src._launch_rays(poses, f32, 1, N_ONLINE)
        render, _ = windows(lambda: eng.render_rays(o1, d1), a.steps, a.repeat, a.warmup)
        got = eng.render_rays(o1, d1)
        check, _ = windows(lambda: eng.spot_check(o1, d1, got), 1, a.repeat, 1)

        def online():
            step[0] += 1
            bo, bd, bt = src.batch(step[0], N_ONLINE)
            bo, bd, bt = (torch.cat([x, pool[:, 3 * k:3 * k + 3]], 0) for k, x in enumerate((bo, bd, bt)))
            torch.cuda.synchronize()                                          # the loop's data_time bracket
            tr.step(bo, bd, bt, 1e-4, 1., t_rand)[0].item()
        t0 = time.perf_counter()
        src.draws(2)
        host_ms = (time.perf_counter() - t0) * 1e3
        on_dev, on_wall = windows(online, a.steps, a.repeat, a.warmup)
        st2, _ = windows(student, a.steps, a.repeat, 1)                    # the student step again, beside this teacher's windows
        ratio = statistics.median(on_wall) / statistics.median(st2)
        lines += [f'{name}, mode chosen by auto: {mode} (probe differences {eng.auto_diffs})',
                  f'  r2l_rand_rays, {N_ONLINE} rays of {N_POSE} poses (incl. the upload of the poses and focals): {fmt(rays, "us", 1e3)}',
                  f'  teacher render of those rays (render_rays, {eng.precision_name}): {fmt(render)} = {N_ONLINE / statistics.median(render) * 1e3:.3e} rays/s',
                  f'  spot check of a batch ({eng.WATCH_RAYS} of its rays against fp16x3; every 100th step by default): {fmt(check)}',
                  f'  host draws of a step ({N_POSE} x pose_spherical + focal; serial with the device: the step waits for them): {host_ms:.2f} ms',
                  f'  online step (source.batch + pool rows + R2LTrainer.step; {src.checks} spot check(s), {len(src.fallbacks)} fallback(s) in '
                  f'{step[0]} steps): {fmt(on_dev)} on the device, {fmt(on_wall)} on the host\'s clock',
                  f'  student step beside it: {fmt(st2)}',
                  f'  online step / shard step = {ratio:.3f} (host clock of the online step over the student step; render + rays alone would '
                  f'add {(statistics.median(render) + statistics.median(rays)) / statistics.median(st2):.3f})']
        eng.close()
    write(lines, a.out)


if __name__ == '__main__':
    main()
