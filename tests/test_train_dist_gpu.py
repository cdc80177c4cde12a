"""GPU: training of the R2L student on several ranks (csrc/r2l_train.hip: r2l_train_sum_parts; flat_trainer.FlatAdam.exchange_gradients;
train.ShardedStep and the loop; online.OnlineTeacherSource.batch(rows=...)).

The loop is replicated and the rays are sharded; the ranks' gradients are added in rank order by one kernel, so a step on N ranks is
what ONE process computes that runs the slices one after the other: the yardstick of the kernel is torch's separate mul and add,
bit for bit, and the yardstick of a 2-rank step is its one-process emulation, bit for bit.  The quality of the sharded gradient is
measured like tests/test_train_gpu.py measures the 1-rank one: against float64 autograd of oracle/r2l_oracle.py's forward.

Two ranks (gloo between them, both on this card) are started ONCE for everything that needs them in-process (`two_ranks`); the
command line runs as `main.py --gpus 2`.  Every child runs under a time limit."""
import ctypes as C
import json
import os
import re
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')
KW = dict(n_sample=4, L=4, netdepth=8, netwidth=64, use_residual=True, trial=dict(body_arch='resmlp'))
STEPS = [(37, 1e-3), (37, 5e-4), (37, 2e-3), (1, 1e-3)]          # (rays, lr): 37 = 19 + 18; 1 = 1 + 0, rank 1 holds nothing
GRAD_N, GRAD_SEEDS = 300, (0, 1, 2, 3)
ONLINE_N, ONLINE_H = 64, 16


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rays(n, seed):
    """tests/test_train_gpu.py's rays: origins (0, 0, 4) + 0.2 N(0, 1), directions normalize(-o + 0.8 N(0, 1))"""
    g = torch.Generator().manual_seed(seed)
    o = torch.tensor([0., 0., 4.]) + 0.2 * torch.randn(n, 3, generator=g)
    d = -o + 0.8 * torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=-1, keepdim=True)
    tgt = 0.5 + 0.5 * torch.sin(3 * d + 2 * o + torch.tensor([0., 1., 2.]))
    return o, d, tgt


def _step_batch(k):
    n = STEPS[k][0]
    ro, rd, tgt = _rays(n, 40 + k)
    t_rand = torch.rand(n, KW['n_sample'], generator=torch.Generator().manual_seed(60 + k))
    return tuple(t.cuda() for t in (ro, rd, tgt, t_rand))


def _grad_batch(seed):
    g = torch.Generator().manual_seed(100 + seed)
    ro, rd, _ = _rays(GRAD_N, seed)
    return ro, rd, torch.rand(GRAD_N, 3, generator=g), torch.rand(GRAD_N, KW['n_sample'], generator=g)


def _grad_state(seed, input_dim):
    from oracle import r2l_oracle as O
    return O.make_v3_2_state(seed, KW['netdepth'], KW['netwidth'], input_dim, '', 'relu', KW['trial'])


def _sum_parts(L, parts, pitch, n_part, weights, count, out):
    w = (C.c_float * len(weights))(*weights)
    rc = L.r2l_train_sum_parts(_p(parts), pitch, n_part, w, count, _p(out), _stream())
    assert rc == 0, L.r2l_last_error().decode()


@pytest.fixture(scope='module')
def L(pkg, built_lib):
    from efficient_nerf_amd import _lib
    return _lib.lib()


# ---- 1. the kernel, bit for bit ----------------------------------------------------------------------------------------------
def _weight_sets(n_part):
    """n_r / n of n = 37 over 2 and 3 ranks (no powers of two), over 8; a set with a zero weight (an empty slice)"""
    split = lambda n, w: [(n // w + (1 if r < n % w else 0)) / n for r in range(w)]
    sets = [split(37, n_part)] if n_part > 1 else [[19 / 37], [1.0]]
    if n_part > 1:
        z = split(37, n_part - 1) + [0.0]
        sets += [z, [0.0] + z[:-1]]
    return sets


def _values(shape, seed):
    """magnitudes over 1e-9 .. 1, every fourth value scaled by 1e-37: its products with the weights are denormal or flush to 0"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g).sign() * 10 ** (-9 * torch.rand(shape, generator=g))
    tiny = torch.rand(shape, generator=g) < 0.25
    return torch.where(tiny, v * 1e-37, v)


@pytest.mark.parametrize('n_part', [1, 2, 3, 8])
@pytest.mark.parametrize('count', [0, 1, 3, 255, 256, 257, 4099])
def test_sum_parts_is_torchs_mul_and_add_bit_for_bit(L, count, n_part):
    """pitch == count and a pitch that breaks the 16-byte alignment of the later parts, an aligned and an unaligned base, out beside
    the parts and out = part 0; nothing is written behind `count` and no other part is touched"""
    odd = count + 1 if (count + 1) % 4 else count + 2
    for case, (pitch, base) in enumerate(((count, 0), (odd, 0), (count + (-count) % 4, 1))):
        for wi, weights in enumerate(_weight_sets(n_part)):
            wt = torch.tensor(weights, dtype=torch.float32)                      # the fp32 the kernel receives by value
            for alias in (False, True):
                buf = torch.full((base + n_part * max(pitch, 1) + count + 8,), -7., device='cuda')
                parts = buf[base:]
                src = _values((n_part, count), 1000 * count + 10 * n_part + case).cuda()
                for k in range(n_part):
                    parts[k * pitch:k * pitch + count] = src[k]
                keep = buf.clone()
                out = parts if alias else torch.full((count + 8,), -7., device='cuda')
                _sum_parts(L, parts, pitch, n_part, wt.tolist(), count, out)
                wd = wt.cuda()
                acc = src[0] * wd[0]
                for r in range(1, n_part):
                    acc = acc + src[r] * wd[r]
                torch.cuda.synchronize()
                assert torch.equal(out[:count], acc), (count, n_part, pitch, base, wi, alias)
                if alias:
                    keep[base:base + count] = acc
                else:
                    assert bool((out[count:] == -7.).all())
                assert torch.equal(buf, keep)
                if count == 4099 and case == 0 and wi == 0 and not alias:
                    prod = src * wd[:, None]                                       # denormal products are among the values added
                    assert bool(((prod != 0) & (prod.abs() < 1.17e-38)).any())


def test_sum_parts_refuses_what_it_cannot_hold(L):
    p = torch.zeros(64, device='cuda')
    w = (C.c_float * 65)(*([1.0] * 65))
    for n_part in (0, 65):
        assert L.r2l_train_sum_parts(_p(p), 0, n_part, w, 0, _p(p), None) == -1 and 'r2l_train_sum_parts' in L.r2l_last_error().decode()
    assert L.r2l_train_sum_parts(_p(p), 4, 2, w, 8, _p(p), None) == -1            # pitch < count
    assert L.r2l_train_sum_parts(_p(p), 8, 2, w, 8, _p(p[4:]), None) == -1        # out inside the parts, not part 0
    assert L.r2l_train_sum_parts(_p(p), 1, 64, w, 1, _p(p), None) == 0            # 64 parts are held
    torch.cuda.synchronize()


# ---- the two ranks -----------------------------------------------------------------------------------------------------------
def _job_steps(rank, T):
    """STEPS on a seeded network through ShardedStep; before the one-ray step rank 1's gradient buffers hold NaNs"""
    tr = T.R2LTrainer(max_rays=19, **KW)
    tr.load_state_dict(T.init_state_dict(tr.plan, seed=3))
    st = T.ShardedStep(tr)
    out = []
    for k, (n, lr) in enumerate(STEPS):
        ro, rd, tgt, t_rand = _step_batch(k)
        if n == 1 and rank == 1:
            tr._grad.fill_(NAN)
            tr._xsend.fill_(NAN)
        loss, err = st.step(ro, rd, tgt, lr, 1., t_rand)
        out.append({k_: v.detach().cpu().clone() for k_, v in (('param', tr._param), ('m', tr._m), ('v', tr._v), ('loss', loss), ('err', err))})
    return out


def _job_grads(rank, T, D):
    """the exchanged gradient of GRAD_N rays on the oracle's networks, seeds GRAD_SEEDS"""
    tr = T.R2LTrainer(max_rays=GRAD_N // 2, **KW)
    r0, r1 = D.row_shard(GRAD_N, rank, 2)
    out = []
    for seed in GRAD_SEEDS:
        tr.load_state_dict(_grad_state(seed, tr.input_dim))
        ro, rd, tgt, t_rand = (t.cuda() for t in _grad_batch(seed))
        tr.forward_backward(ro[r0:r1], rd[r0:r1], tgt[r0:r1], 1., t_rand[r0:r1])
        loss, _ = tr.exchange_gradients(None, r1 - r0, GRAD_N)
        out.append(({k: v.cpu() for k, v in tr.grads().items()}, float(loss.item())))
    return out


def _job_guard(rank, T, out_dir):
    """two iterations with a checkpoint after each; rank 1's first parameter moves after the first step"""
    from efficient_nerf_amd import frontend as fe
    from efficient_nerf_amd._lib import R2LError
    args = fe.parse_args(['--N_iters', '2', '--i_weights', '1', '--i_print', '1', '--i_testset', '0'])
    tr = T.R2LTrainer(max_rays=19, **KW)
    tr.load_state_dict(T.init_state_dict(tr.plan, seed=4))
    tr.check_agreement(None)                                     # equal weights pass
    batch = _step_batch(0)[:3]
    wdir = os.path.join(out_dir, 'guard_weights')
    os.makedirs(wdir, exist_ok=True)
    torch.manual_seed(9)                                         # the step draws t_rand: the same on both ranks
    lines = []

    def after_step(_batch, _err):
        if rank == 1:
            tr._param[0] += 1.0

    try:
        T.run_iterations(args, T.ShardedStep(tr), 0, (0, 0), wdir, lines.append, draw=lambda i: batch, after_step=after_step,
                         writer=rank == 0, guard=lambda it: tr.check_agreement(None, f' by iteration {it}'))
    except R2LError as e:
        return {'raised': str(e), 'lines': lines}
    return {'raised': None, 'lines': lines}


def _job_online(rank, D):
    """a synthetic teacher behind OnlineTeacherSource: an unwatched step whole and sharded; then a watched step on which rank 1's
    spot check (a stub) misses once"""
    from efficient_nerf_amd import NeRFEngine, PREC_FP16_FP8
    from efficient_nerf_amd.online import OnlineTeacherSource
    from oracle import r2l_oracle as O
    H = ONLINE_H
    focal = O.focal_from_angle(H)
    eng = NeRFEngine(H, H, focal, precision=PREC_FP16_FP8).load_state_dicts(O.make_teacher_state(3), O.make_teacher_state(4))
    lines = []
    src = OnlineTeacherSource(eng, H, H, focal, n_pose=3, seed=3, watch_every=2, log=lines.append)
    rows = D.row_shard(ONLINE_N, rank, 2)
    whole = [t.cpu().clone() for t in src.batch(3, ONLINE_N)]
    shard = [t.cpu().clone() for t in src.batch(3, ONLINE_N, rows=rows)]
    calls = []

    def spot_check(ro, rd, got):
        calls.append(ro.shape[0])
        return (not (rank == 1 and len(calls) == 1)), {'rgb': 1.0 if rank == 1 else 0.0}

    eng.spot_check = spot_check
    before = eng.precision_name
    missed = [t.cpu().clone() for t in src.batch(4, ONLINE_N, rows=rows)]
    after = eng.precision_name
    own = eng.render_rays(missed[0].cuda(), missed[1].cuda())['rgb_map'].cpu()       # all rows, in the mode both ended in
    res = {'whole': whole, 'shard': shard, 'missed': missed, 'own': own, 'modes': (before, after), 'fallbacks': list(src.fallbacks),
           'calls': calls, 'lines': lines}
    eng.close()
    return res


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      R2L_DIST_BACKEND='gloo')
    import _pkg
    _pkg.load()
    import torch.distributed as dist
    from efficient_nerf_amd import dist as D, train as T
    D.init()
    torch.cuda.set_device(D.local_device(rank))
    res = {'steps': _job_steps(rank, T), 'grads': _job_grads(rank, T, D), 'guard': _job_guard(rank, T, out_dir), 'online': _job_online(rank, D)}
    torch.save(res, os.path.join(out_dir, f'r{rank}.pt'))
    D.barrier_sync()
    dist.destroy_process_group()


@pytest.fixture(scope='module')
def two_ranks(pkg, built_lib, tmp_path_factory):
    import torch.multiprocessing as mp
    out_dir = str(tmp_path_factory.mktemp('train_dist'))
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.spawn(_worker, args=(2, port, out_dir), nprocs=2, join=False)
    t_end = time.monotonic() + 240
    try:
        while not ctx.join(timeout=0.5):                                 # raises when a rank failed, and stops the other
            assert time.monotonic() < t_end, 'the two ranks did not finish in 240 s'
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    return [torch.load(os.path.join(out_dir, f'r{k}.pt'), weights_only=False) for k in range(2)], out_dir


# ---- 2. a 2-rank step equals its one-process emulation -----------------------------------------------------------------------
def test_two_rank_steps_equal_their_one_process_emulation(L, two_ranks):
    from efficient_nerf_amd import dist as D, train as T
    r = [x['steps'] for x in two_ranks[0]]
    tr = T.R2LTrainer(max_rays=37, **KW)
    tr.load_state_dict(T.init_state_dict(tr.plan, seed=3))
    P = tr.n_param
    for k, (n, lr) in enumerate(STEPS):
        ro, rd, tgt, t_rand = _step_batch(k)
        parts = torch.zeros((2, P), device='cuda')
        losses, errs, weights = [], [], []
        for rank in range(2):
            r0, r1 = D.row_shard(n, rank, 2)
            weights.append((r1 - r0) / n)
            if r1 == r0:                                                 # an empty slice: exact zeros
                losses.append(torch.zeros(1, device='cuda'))
                continue
            losses.append(tr.forward_backward(ro[r0:r1], rd[r0:r1], tgt[r0:r1], 1., t_rand[r0:r1]).clone())
            parts[rank] = tr._grad
            errs.append(tr._err[:r1 - r0].clone())
        _sum_parts(L, parts, P, 2, weights, P, tr._grad)
        tr.adam(lr)
        wt = torch.tensor(weights, dtype=torch.float32).cuda()
        loss = losses[0] * wt[0] + losses[1] * wt[1]
        torch.cuda.synchronize()
        for name, mine in (('param', tr._param), ('m', tr._m), ('v', tr._v), ('loss', loss), ('err', torch.cat(errs))):
            assert torch.equal(r[0][k][name], r[1][k][name]), (k, name)
            assert torch.equal(r[0][k][name], mine.cpu()), (k, name)
        assert r[0][k]['err'].shape == (n,) and torch.isfinite(r[0][k]['param']).all() and torch.isfinite(r[0][k]['loss']).all()
    assert not torch.equal(r[0][0]['param'], r[0][3]['param'])           # and the steps moved the weights


# ---- 3. the sharded gradient is as good as the 1-rank one --------------------------------------------------------------------
def _autograd(forward, sd, emb, target, dtype):
    prm = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    loss = ((forward(prm, emb.to(dtype)) - target.to(dtype)) ** 2).mean()
    loss.backward()
    return loss.item(), {k: v.grad.detach() for k, v in prm.items()}


def _gap(got, ref):
    """relative L2 gap of the whole-network gradient from the float64 one"""
    num = sum(float((got[k].double().cpu() - ref[k]).norm()) ** 2 for k in ref)
    return np.sqrt(num) / np.sqrt(sum(float(ref[k].norm()) ** 2 for k in ref))


def test_sharded_gradient_is_as_close_to_float64_as_the_one_rank_gradient(two_ranks):
    """per seed: gap of the 2-rank gradient <= 2 x the largest 1-rank gap over the seeds (another realisation of the same rounding:
    two shorter reductions and one weighted addition)"""
    from efficient_nerf_amd import train as T
    from oracle import r2l_oracle as O
    tr = T.R2LTrainer(max_rays=GRAD_N, **KW)
    fwd = lambda prm, x: O.v3_2_forward(prm, x, KW['netdepth'], 'relu', True, KW['trial'])
    gap1, gap2 = [], []
    for i, seed in enumerate(GRAD_SEEDS):
        sd = _grad_state(seed, tr.input_dim)
        tr.load_state_dict(sd)
        ro, rd, tgt, t_rand = _grad_batch(seed)
        emb = tr.embed(ro.cuda(), rd.cuda(), 1., t_rand.cuda()).cpu()
        tr.forward_backward(ro.cuda(), rd.cuda(), tgt.cuda(), 1., t_rand.cuda())
        l64, g64 = _autograd(fwd, sd, emb, tgt, torch.float64)
        g2, loss2 = two_ranks[0][0]['grads'][i]
        assert all(torch.equal(g2[k], two_ranks[0][1]['grads'][i][0][k]) for k in g2)
        assert set(g2) == set(g64)
        gap1.append(_gap(tr.grads(), g64))
        gap2.append(_gap(g2, g64))
        assert abs(loss2 - l64) <= 1e-4 * l64          # a sanity line (a wrong weight is a percent-level error), not the yardstick
    print(f'relative L2 gap of the gradient from float64, seeds {GRAD_SEEDS}: 1 rank {[f"{g:.2e}" for g in gap1]}, 2 ranks {[f"{g:.2e}" for g in gap2]}')
    for g in gap2:
        assert g <= 2 * max(gap1)


# ---- 4. the loop on 2 ranks --------------------------------------------------------------------------------------------------
def test_diverged_weights_raise_on_both_ranks_and_write_nothing(two_ranks):
    r, out_dir = two_ranks
    for k in range(2):
        msg = r[k]['guard']['raised']
        assert msg and 'diverged' in msg and 'iteration 1' in msg and 'rank(s) [1]' in msg, msg
        assert not any('Save checkpoint' in ln for ln in r[k]['guard']['lines'])
    assert os.listdir(os.path.join(out_dir, 'guard_weights')) == []


def test_online_targets_are_gathered_and_the_ranks_step_down_together(two_ranks):
    r = [x['online'] for x in two_ranks[0]]
    for k in range(2):
        assert all(t.shape == (ONLINE_N, 3) for t in r[k]['shard'])
        assert all(torch.equal(a, b) for a, b in zip(r[k]['whole'], r[k]['shard']))          # rays and gathered targets = one rank's batch
    assert all(torch.equal(a, b) for a, b in zip(r[0]['shard'], r[1]['shard']))
    # the forced miss on rank 1: both step down once, one line (rank 0's), equal batches rendered in the mode they ended in
    for k in range(2):
        assert r[k]['modes'] == ('fp16_fp8', 'fp16_mix') and len(r[k]['fallbacks']) == 1 and r[k]['fallbacks'][0]['step'] == 4
        assert r[k]['calls'] == [ONLINE_N // 2] * 2                                          # each rank checks its own rows, twice
        assert torch.equal(r[k]['missed'][2], r[k]['own'])
    assert all(torch.equal(a, b) for a, b in zip(r[0]['missed'], r[1]['missed']))
    lines = [[ln for ln in r[k]['lines'] if ln.startswith('[precision] step 4:')] for k in range(2)]
    assert len(lines[0]) == 1 and 'fp16_fp8' in lines[0][0] and '-> fp16_mix' in lines[0][0] and lines[1] == []


SIZE, N_TRAIN, N_TEST, ANGLE = 16, 32, 3, 0.6911
NET = ['--model_name', 'R2L', '--dataset_type', 'blender', '--white_bkgd', '--testskip', '1', '--netdepth', '8', '--netwidth', '64',
       '--n_sample_per_ray', '4', '--multires', '4', '--use_residual', '--trial.ON', '--trial.body_arch', 'resmlp']
TRAIN = ['--data_mode', 'rays', '--N_rand', '2', '--N_iters', '6', '--i_print', '1', '--i_weights', '3', '--i_testset', '3', '--hard_ratio', '0.2',
         '--hard_mul', '2']


@pytest.fixture(scope='module')
def scene(pkg, built_lib, tmp_path_factory):
    """tests/test_train_eval_gpu.py's scene: 16 x 16 RGBA views of a soft-edged disc, 32 train views (two shards of 4096 rays from
    convert_data) and three test views"""
    from efficient_nerf_amd import convert_data as CD
    from efficient_nerf_amd.frontend import pose_spherical, write_png
    root = tmp_path_factory.mktemp('train_dist_cli')
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
    return {'root': str(root), 'datadir': str(d), 'shards': f'{d}_real_train'}


def _argv(scene, expname, extra=()):
    return NET + TRAIN + ['--datadir', scene['datadir'], '--datadir_kd', scene['shards'], '--basedir', scene['root'], '--expname', expname] + list(extra)


def _main(scene, argv, seconds=240):
    env = dict(os.environ, R2L_DIST_BACKEND='gloo')
    return subprocess.run(['timeout', '-k', '10', str(seconds), sys.executable, os.path.join(ROOT, 'main.py')] + argv, cwd=scene['root'],
                          capture_output=True, text=True, env=env)


def _two_rank_run(scene, expname, extra=()):
    r = _main(scene, ['--gpus', '2', '--launch_timeout', '200', '--dist_seed', '5'] + _argv(scene, expname, extra))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout, r.stderr


def _state(scene, expname, name='ckpt.tar'):
    ck = torch.load(os.path.join(scene['root'], expname, 'weights', name), map_location='cpu', weights_only=False)
    return ck['network_fn_state_dict'], ck['optimizer_state_dict']['state'], ck


def test_cli_on_two_ranks_with_the_hard_ray_pool(scene):
    """main.py --gpus 2 on ray shards with --hard_ratio 0.2 --hard_mul 2 (8192 rays per step; the pool collects 1638 rows a step):
    rank 0 alone logs and writes, twice the same command gives the same bits, and the checkpoint renders"""
    out, errs = _two_rank_run(scene, 'a')
    both = out.splitlines() + errs.splitlines()
    for k in range(1, 7):
        assert sum(ln.startswith(f'[TRAIN] Iter {k} ') for ln in both) == 1 == sum(ln.startswith(f'[TRAIN] Iter {k} ') for ln in out.splitlines())
    for k in (3, 6):
        assert sum(ln.startswith(f'[TEST] Iter {k} ') for ln in both) == 1
    assert sum(ln.startswith('[TEST] Iter') for ln in both) == 2 and sum(ln.startswith('[TRAIN] Iter') for ln in both) == 6
    start = [ln for ln in both if ln.startswith('Found 2 shard(s)')]
    assert len(start) == 1 and start[0].endswith('; 2 ranks, ≤ 4915 rays each') and '2 per step + 1638 hard rays' in start[0], start
    losses = [float(ln.split(' loss ')[1].split()[0]) for ln in out.splitlines() if ln.startswith('[TRAIN] Iter')]
    assert np.isfinite(losses).all()
    assert sorted(os.listdir(os.path.join(scene['root'], 'a', 'weights'))) == ['ckpt.tar', 'ckpt_best.tar']       # and no .tmp
    for it in (3, 6):
        assert sorted(os.listdir(os.path.join(scene['root'], 'a', f'testset_iter{it}'))) == [f'{k:03d}.png' for k in range(N_TEST)]
    # the same command again
    _two_rank_run(scene, 'b')
    (wa, sa, cka), (wb, sb, _) = _state(scene, 'a'), _state(scene, 'b')
    assert cka['global_step'] == 6 and list(wa) == list(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
    assert sorted(sa) == sorted(sb) and len(sa) > 0 and all(torch.equal(sa[k][m], sb[k][m]) for k in sa for m in ('exp_avg', 'exp_avg_sq', 'step'))
    wbest = _state(scene, 'a', 'ckpt_best.tar')[2]
    assert wbest['best_psnr'] > 0 and wbest['best_psnr_step'] in (3, 6)
    # the checkpoint renders
    r = _main(scene, NET + ['--datadir', scene['datadir'], '--render_only', '--render_test', '--precision', 'fp32', '--pretrained_ckpt',
                            os.path.join(scene['root'], 'a', 'weights', 'ckpt.tar'), '--basedir', scene['root'], '--expname', 'render'])
    assert r.returncode == 0 and re.search(r'^\[TEST\] TestPSNR (\S+) TestPSNRv2 (\S+) TestSSIM (\S+)$', r.stdout, re.M), r.stdout[-3000:] + r.stderr[-3000:]


def test_cli_on_two_ranks_once_the_pool_is_full(scene):
    """--hard_mul 0.5: the pool holds 4096 rows after three steps, steps 4 to 6 carry 8192 + 1638 rays cut 4915 / 4915"""
    out, _ = _two_rank_run(scene, 'full', extra=['--hard_mul', '0.5', '--i_testset', '0'])
    losses = [float(ln.split(' loss ')[1].split()[0]) for ln in out.splitlines() if ln.startswith('[TRAIN] Iter')]
    assert len(losses) == 6 and np.isfinite(losses).all()
    assert os.listdir(os.path.join(scene['root'], 'full', 'weights')) == ['ckpt.tar'] and _state(scene, 'full')[2]['global_step'] == 6


# ---- 5. one rank is untouched ------------------------------------------------------------------------------------------------
def test_one_rank_enters_no_collective_and_seeds_nothing(scene, monkeypatch):
    import torch.distributed as td
    from efficient_nerf_amd import train as T
    from efficient_nerf_amd.frontend import parse_args

    def refuse(*a, **k):
        raise AssertionError('a collective on one rank')

    for name in ('all_gather_into_tensor', 'all_gather', 'all_reduce', 'broadcast', 'broadcast_object_list', 'all_gather_object'):
        monkeypatch.setattr(td, name, refuse)
    np.random.seed(11)
    torch.manual_seed(11)
    seeded = []
    monkeypatch.setattr(np.random, 'seed', lambda *a, **k: seeded.append('numpy'))
    monkeypatch.setattr(torch, 'manual_seed', lambda *a, **k: seeded.append('torch'))
    lines = []
    T.train(parse_args(_argv(scene, 'one', extra=['--N_iters', '2', '--i_weights', '2', '--i_testset', '2'])), log=lines.append)
    assert seeded == [] and not td.is_initialized()
    start = [ln for ln in lines if ln.startswith('Found 2 shard(s)')]
    assert len(start) == 1 and 'ranks' not in start[0]
    assert sum(ln.startswith('[TRAIN] Iter') for ln in lines) == 2 and sum(ln.startswith('[TEST] Iter') for ln in lines) == 1
    assert sorted(os.listdir(os.path.join(scene['root'], 'one', 'weights'))) == ['ckpt.tar', 'ckpt_best.tar']
