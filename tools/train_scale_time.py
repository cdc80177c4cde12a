#!/usr/bin/env python
"""What a training step of the R2L student costs on 1, 2, 4 and 8 ranks (train.ShardedStep: the loop replicated, the rays sharded,
the ranks' gradients added in rank order), at the README batch: 20 shards of 4,096 rays + 16,384 rows of the hard-ray pool = 98,304
rays through a W256D88 student; and the same under --kd_online (81,920 rays of 100 random 400 x 400 poses from a synthetic teacher).

For every world size the box has cards for, the ranks are started as fresh processes (launch.py; RCCL between them unless
R2L_DIST_BACKEND says otherwise) and rank 0 reports, per step: the step time (HIP events), rays/s, the exchange's share (one
all-gather of [gradient | loss | per-ray error] + r2l_train_sum_parts, timed on its own), the replicated host work that bounds the
scaling (shard path: reading and concatenating 20 shards = the loop's data_time; online path: the pose draws), and the ratio to the
1-rank step of profiles/train_step_time.txt.  World sizes beyond the box's cards are listed as unmeasured (with R2L_DIST_BACKEND=gloo
they run as a rehearsal on shared cards, marked as such).  On any box the kernel of
the ordered sum is timed alone for 1, 2, 4 and 8 parts of the student's 5.9 M parameters.

Windows of --steps repetitions, --repeat windows per quantity after --warmup untimed repetitions; a line gives the median window and
the spread (smallest .. largest window), per repetition.  Writes profiles/train_scale_time.txt.

    python tools/train_scale_time.py [--steps 10] [--repeat 5] [--warmup 3] [--worlds 1,2,4,8] [--out profiles/train_scale_time.txt]
"""
import argparse
import importlib.util
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RAND, SPLIT, N_POOL, N_POSE, HW = 20, 4096, 16384, 100, 400
N_ONLINE = N_RAND * SPLIT


def fmt(ms, unit='ms', scale=1.):
    return f'{statistics.median(ms) * scale:.2f} {unit} ({min(ms) * scale:.2f} .. {max(ms) * scale:.2f})'


def rank_main(a):
    """one rank of a measurement; rank 0 writes its figures to a.json"""
    sys.path.insert(0, ROOT)
    import ctypes as C
    import numpy as np
    import torch
    import _pkg
    _pkg.load()
    from efficient_nerf_amd import NeRFEngine, PRECISIONS, dist as D
    from efficient_nerf_amd._lib import check, current_stream, dptr, lib
    from efficient_nerf_amd.create_data import BlenderDataset_v2, choose_precision_for_rand
    from efficient_nerf_amd.online import OnlineTeacherSource
    from efficient_nerf_amd.train import R2LTrainer, ShardedStep, init_state_dict
    from oracle import r2l_oracle as O
    rank, local_rank, world = D.init()
    torch.cuda.set_device(D.local_device(local_rank))
    D.seed_all(0)

    def windows(fn, steps=a.steps, repeat=a.repeat, warmup=a.warmup):
        for _ in range(warmup):
            fn()
        dev, wall = [], []
        for _ in range(repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            D.barrier_sync()                                  # the ranks enter a window together
            t0 = time.perf_counter()
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3 / steps)
            dev.append(e0.elapsed_time(e1) / steps)
        return dev, wall

    n = N_ONLINE + N_POOL
    res = {'world': world, 'cards': torch.cuda.device_count(), 'backend': torch.distributed.get_backend() if world > 1 else 'none', 'n': n}
    tr = R2LTrainer(netdepth=88, netwidth=256, use_residual=True, trial=dict(body_arch='resmlp'), max_rays=-(-n // world))
    tr.load_state_dict(init_state_dict(tr.plan, seed=0))
    res['n_param'], res['max_rays'] = tr.n_param, tr.max_rays
    stepper = ShardedStep(tr) if world > 1 else tr
    g = torch.Generator().manual_seed(0)
    ro = (torch.tensor([0., 0., 4.]) + 0.2 * torch.randn(n, 3, generator=g)).cuda()
    rd = torch.nn.functional.normalize(-ro.cpu() + 0.8 * torch.randn(n, 3, generator=g), dim=-1).cuda()
    tgt = torch.rand(n, 3, generator=g).cuda()
    pool = torch.cat([ro[:N_POOL], rd[:N_POOL], tgt[:N_POOL]], -1)
    # ---- the shard path: the step on given rays (t_rand drawn by the step, as the loop has it), then the exchange alone
    res['step'], res['step_wall'] = windows(lambda: stepper.step(ro, rd, tgt, 1e-4, 1.)[0].item())
    if world > 1:
        r0, r1 = D.row_shard(n, rank, world)
        res['exchange'], _ = windows(lambda: tr.exchange_gradients(None, r1 - r0, n))
    if rank == 0 and world == 1:          # the ordered sum alone, for the part counts of 1 .. 8 ranks
        res['sum_parts'] = {}
        for parts in (1, 2, 4, 8):
            buf = torch.randn((parts, tr.n_param), generator=g).cuda()
            out = torch.empty(tr.n_param, device='cuda')
            w = (C.c_float * parts)(*([1. / parts] * parts))
            res['sum_parts'][parts], _ = windows(lambda: check(lib().r2l_train_sum_parts(dptr(buf), tr.n_param, parts, w, tr.n_param, dptr(out),
                                                                                       current_stream())), 200 * a.steps)
    # ---- the replicated host work of the shard path: 20 shards read, concatenated and uploaded (every rank does all of it)
    with tempfile.TemporaryDirectory() as d:
        rs = np.random.RandomState(rank)
        for k in range(N_RAND + 4):
            np.save(os.path.join(d, f'train_{k}.npy'), rs.rand(SPLIT, 9).astype(np.float32))
        ds = BlenderDataset_v2(d, dim_dir=3, dim_rgb=3, pseudo_ratio=-1)

        def assemble():
            items = [ds[k] for k in range(N_RAND)]
            return [torch.cat([it[c] for it in items], 0).cuda() for c in range(3)]
        _, res['assemble_wall'] = windows(assemble)
    # ---- the online path: a synthetic teacher in the mode auto picks, the batch (targets of this rank's rows, gathered), pool rows, step
    focal = O.focal_from_angle(HW)
    eng = NeRFEngine(HW, HW, focal, precision=PRECISIONS['fp16x3']).load_state_dicts(O.make_teacher_state(1), O.make_teacher_state(2))
    res['teacher_mode'] = choose_precision_for_rand(eng, HW, HW, focal)
    if world > 1:
        from efficient_nerf_amd.online import agree_teacher_precision
        agree_teacher_precision(eng)
    src = OnlineTeacherSource(eng, HW, HW, focal, n_pose=N_POSE, seed=0, watch_every=100, log=lambda *x: None)
    rows = D.row_shard(N_ONLINE, rank, world) if world > 1 else None
    step = [0]
    data = []

    def online():
        step[0] += 1
        t0 = time.perf_counter()
        bo, bd, bt = src.batch(step[0], N_ONLINE, rows=rows)
        bo, bd, bt = (torch.cat([x, pool[:, 3 * k:3 * k + 3]], 0) for k, x in enumerate((bo, bd, bt)))
        torch.cuda.synchronize()                              # the loop's data_time bracket
        data.append((time.perf_counter() - t0) * 1e3)
        stepper.step(bo, bd, bt, 1e-4, 1.)[0].item()
    res['online'], res['online_wall'] = windows(online)
    res['online_data'] = data[-a.steps * a.repeat:]
    t0 = time.perf_counter()
    for k in range(5):
        src.draws(1000 + k)
    res['draws_ms'] = (time.perf_counter() - t0) * 1e3 / 5
    eng.close()
    if rank == 0:
        with open(a.json, 'w') as f:
            json.dump(res, f)
    D.barrier_sync()
    if world > 1:
        torch.distributed.destroy_process_group()


def report(results, worlds, a):
    med = statistics.median
    r1 = results.get(1)
    cards = r1['cards'] if r1 else 0
    n = N_ONLINE + N_POOL
    parent = None
    try:
        with open(os.path.join(ROOT, 'profiles', 'train_step_time.txt')) as f:
            parent = float(re.search(r'^step: (\S+) ms', f.read(), re.M).group(1))
    except (OSError, AttributeError):
        pass
    lines = [f'Training step of the R2L student on several ranks at the README batch: {N_RAND} shards of {SPLIT} rays + {N_POOL} hard-ray rows = {n} '
             f'rays, W256D88; this box has {cards} card(s); HIP events, median of {a.repeat} windows of {a.steps} repetitions after {a.warmup} '
             f'warm-up repetitions (smallest .. largest window)']
    for w in worlds:
        r = results.get(w)
        if r is None:
            lines.append(f'{w} rank(s): unmeasured' + (f' (the box has {cards} card(s))' if w > cards else ' (the run failed)'))
            continue
        st = med(r['step'])
        lines.append(f"{w} rank(s) ({r['backend']}), <= {r['max_rays']} rays each:" +
                     (' -- A REHEARSAL: the ranks share cards and exchange through the host, no figure below is a measurement' if w > cards else ''))
        lines.append(f"  shard path, step on given rays: {fmt(r['step'])} = {n / st * 1e3:.3e} rays/s" +
                     (f'; / the 1-rank step of profiles/train_step_time.txt ({parent:.2f} ms) = {st / parent:.3f}' if parent else '') +
                     (f"; / this run's 1-rank step = {st / med(r1['step']):.3f}" if r1 and w > 1 else ''))
        if 'exchange' in r:
            ex = med(r['exchange'])
            lines.append(f"    exchange (all-gather of {w} x {4 * (r['n_param'] + 1 + r['max_rays']) / 1e6:.1f} MB + the ordered sum): {fmt(r['exchange'])} = "
                         f'{ex / st:.3f} of the step')
        asm = med(r['assemble_wall'])
        lines.append(f"    replicated on the host: {N_RAND} shards read, concatenated, uploaded (the loop's data_time): {fmt(r['assemble_wall'])}; with it a "
                     f'step is {st + asm:.2f} ms = {n / (st + asm) * 1e3:.3e} rays/s' +
                     (f", {(med(r1['step']) + med(r1['assemble_wall'])) / (st + asm):.2f} x the 1-rank loop" if r1 and w > 1 else ''))
        on = med(r['online_wall'])
        lines.append(f"  online path (synthetic teacher in {r['teacher_mode']}), batch + pool rows + step: {fmt(r['online'])} on the device, "
                     f"{fmt(r['online_wall'])} on the host's clock = {n / on * 1e3:.3e} rays/s" +
                     (f", {med(r1['online_wall']) / on:.2f} x the 1-rank online step" if r1 and w > 1 else ''))
        lines.append(f"    data_time (poses, rays, this rank's targets, the gather, pool rows): {fmt(r['online_data'])}; of it replicated on the host: "
                     f"the pose draws, {r['draws_ms']:.2f} ms")
    if r1 and 'sum_parts' in r1:
        lines.append(f"r2l_train_sum_parts alone on one card, {r1['n_param']} floats per part: " + '; '.join(
            f"{p} part(s) {fmt(v, 'us', 1e3)} = {4 * r1['n_param'] * (int(p) + 1) / med(v) / 1e6:.0f} GB/s" for p, v in sorted(r1['sum_parts'].items(), key=lambda kv: int(kv[0]))))
    missing = [w for w in worlds if w not in results]
    if missing:
        lines.append(f'Unmeasured: {missing} rank(s) -- the all-gather over xGMI, the exchange\'s share and the speed-up on several cards.')
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--repeat', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--worlds', type=str, default='1,2,4,8')
    ap.add_argument('--out', type=str, default=os.path.join(ROOT, 'profiles', 'train_scale_time.txt'))
    ap.add_argument('--limit', type=float, default=900., help='seconds a measurement may take')
    ap.add_argument('--json', type=str, default='', help='(a rank of a measurement: where rank 0 writes its figures)')
    a = ap.parse_args()
    if a.json:
        return rank_main(a)
    spec = importlib.util.spec_from_file_location('r2l_launch', os.path.join(ROOT, 'efficient-nerf_amd', 'launch.py'))
    launch = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(launch)
    worlds = sorted({int(w) for w in a.worlds.split(',')} | {1})
    results = {}
    me = os.path.abspath(__file__)
    with tempfile.TemporaryDirectory() as d:
        for w in worlds:
            if w > 1 and w > results.get(1, {}).get('cards', 0) and os.environ.get('R2L_DIST_BACKEND') != 'gloo':
                continue          # (under the gloo rehearsal the ranks share cards: the lines are marked as no measurement)
            path = os.path.join(d, f'w{w}.json')
            argv = ['--steps', str(a.steps), '--repeat', str(a.repeat), '--warmup', str(a.warmup), '--json', path]
            if w == 1:
                env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE')}
                try:
                    rc = subprocess.run([sys.executable, me] + argv, env=env, timeout=a.limit).returncode
                except subprocess.TimeoutExpired:
                    rc = 124
            else:
                rc = launch.spawn_ranks(me, argv, w, timeout=a.limit)
            if rc == 0 and os.path.exists(path):
                with open(path) as f:
                    results[w] = json.load(f)
            else:
                print(f'[train_scale_time] {w} rank(s): exit code {rc}', file=sys.stderr)
                if w == 1:
                    raise SystemExit(rc or 1)
    results = {int(k): v for k, v in results.items()}
    for r in results.values():
        if 'sum_parts' in r:
            r['sum_parts'] = {int(k): v for k, v in r['sum_parts'].items()}
    text = report(results, worlds, a)
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
