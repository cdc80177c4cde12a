"""CPU: the parts of student training that need no device -- the command line, the learning-rate schedule, the hard-ray pool's
bookkeeping, the argument checks of the new C-ABI entry points, and the optimizer state's format (it must load into a real
torch.optim.Adam and come back)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R2L_EINVAL = -1

README_CMD = ['--model_name', 'R2L', '--config', os.path.join(ROOT, 'configs', 'lego_noview.txt'), '--n_sample_per_ray', '16',
              '--netwidth', '256', '--netdepth', '88', '--datadir_kd', 'DIR', '--N_iters', '1200000', '--N_rand', '20', '--data_mode', 'rays',
              '--hard_ratio', '0.2', '--hard_mul', '20', '--use_residual', '--trial.ON', '--trial.body_arch', 'resmlp',
              '--warmup_lr', '0.0001,200']


def test_readme_training_command_parses(pkg):
    from efficient_nerf_amd import frontend as fe
    a = fe.parse_args(README_CMD)
    assert not a.render_only and a.model_name == 'R2L' and a.data_mode == 'rays'
    assert (a.N_iters, a.N_rand, a.netdepth, a.netwidth, a.n_sample_per_ray) == (1200000, 20, 88, 256, 16)
    assert a.hard_ratio == '0.2' and a.hard_mul == 20 and a.warmup_lr == '0.0001,200' and a.datadir_kd == 'DIR'
    assert a.trial.ON and a.trial.body_arch == 'resmlp' and a.use_residual
    # the defaults of the reference's option.py
    d = fe.parse_args([])
    assert (d.N_iters, d.lrate, d.warmup_lr, d.hard_ratio, d.hard_mul, d.datadir_kd, d.pseudo_ratio, d.data_mode, d.i_print, d.i_weights,
            d.resume, d.N_rand, d.lrate_decay) == (200000, 5e-4, '', '', 1, '', -1., 'images', 100, 10000, False, 4096, 250)
    assert fe.parse_args(['--num_worker', '4']).num_workers == 4 and d.num_workers == 8


def test_teacher_training_is_refused(pkg):
    from efficient_nerf_amd import frontend as fe
    with pytest.raises(SystemExit) as e:
        fe.main(['--model_name', 'nerf', '--config', os.path.join(ROOT, 'configs', 'lego.txt')])
    assert 'teacher training is not built' in str(e.value)


def test_learning_rate_schedule_closed_form(pkg):
    from efficient_nerf_amd.train import learning_rate
    lrate, start, end, decay = 5e-4, 1e-4, 200., 500
    for step in (1, 100, 199, 200, 201, 10 ** 5):
        if step < end:
            want = start + (lrate - start) * step / end
        else:
            want = lrate * 10. ** (-(step - end) / (decay * 1000.))
        got = learning_rate(step, lrate, decay, '0.0001,200')
        assert abs(got - want) <= 1e-12 * want, (step, got, want)
    assert learning_rate(199, lrate, decay, '0.0001,200') < lrate == learning_rate(200, lrate, decay, '0.0001,200')
    assert learning_rate(250000, lrate, 250) == pytest.approx(lrate * 0.1, rel=1e-12)       # no warm-up: main.py:1193


def test_hard_pool_bookkeeping(pkg):
    from efficient_nerf_amd.train import HardRayPool
    B, mul = 50, 2
    for ratio, n_in, n_out in (('0.2', 10, 10), ('0.1,0.3', 5, 15), ('0.4,0.2', 10, 10)):
        pool = HardRayPool(ratio, mul)
        assert pool.counts(B) == (n_in, n_out)               # n_hard_in <= n_hard_out
        np.random.seed(3)
        g = torch.Generator().manual_seed(0)
        step = 0
        while not pool.full:                                 # fill: the batch's n_in worst rays are appended until B * mul rows
            assert pool.draw(B) is None
            ro, rd, tg = (torch.rand(B, 3, generator=g) + step for _ in range(3))
            err = torch.rand(B, generator=g)
            before = 0 if pool.rows is None else pool.rows.shape[0]
            pool.update(err, ro, rd, tg, B)
            worst = torch.sort(err)[1][-n_in:]
            assert pool.rows.shape == (before + n_in, 9)
            assert torch.equal(pool.rows[before:], torch.cat([ro[worst], rd[worst], tg[worst]], -1))
            step += 1
            assert step <= B * mul
        assert pool.rows.shape[0] >= B * mul > pool.rows.shape[0] - n_in
        size = pool.rows.shape[0]
        for _ in range(3):                                   # full: n_out rows drawn, n_in of those drawn replaced
            old = pool.rows.clone()
            picked = pool.draw(B)
            ix = pool._ix_out.copy()
            assert picked.shape == (n_out, 9) and len(set(ix.tolist())) == n_out and torch.equal(picked, old[ix])
            ro, rd, tg = (torch.rand(B + n_out, 3, generator=g) + 100 for _ in range(3))
            err = torch.rand(B + n_out, generator=g)
            err[B:] = 9.                                     # the drawn rays themselves are never candidates (rgb[:batch_size])
            pool.update(err, ro, rd, tg, B)
            worst = torch.sort(err[:B])[1][-n_in:]
            assert pool.rows.shape[0] == size
            assert torch.equal(pool.rows[ix[:n_in]], torch.cat([ro[worst], rd[worst], tg[worst]], -1))
            keep = np.setdiff1d(np.arange(size), ix[:n_in])
            assert torch.equal(pool.rows[keep], old[keep])


def test_new_entry_points_check_their_arguments(pkg, built_lib):
    """R2L_EINVAL with a message on NULL or bad arguments, before any device is looked for"""
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    err = lambda: L.r2l_last_error().decode()
    p = C.c_void_p(0x1000)
    q = C.c_void_p(0x100000)
    assert L.r2l_linear_forward_dev(None, p, 4, 4, p, 4, 1, q, 4, None, 0, 1.0, 0, None, 0, None) == R2L_EINVAL and 'r2l_linear_forward_dev' in err()
    assert L.r2l_linear_forward_dev(p, p, 4, 4, p, 3, 1, q, 4, None, 0, 1.0, 0, None, 0, None) == R2L_EINVAL      # ldx < in_dim
    assert L.r2l_linear_forward_dev(p, p, 4, 4, p, 4, 1, q, 4, None, 0, 1.0, 7, None, 0, None) == R2L_EINVAL      # unknown activation
    assert L.r2l_linear_forward_dev(p, p, 4, 4, q, 4, 2, q, 4, None, 0, 1.0, 0, None, 0, None) == R2L_EINVAL and 'overlap' in err()
    assert L.r2l_train_act_backward(None, 4, p, 4, None, 0, 1, 4, 1, 1.0, q, 4, None, 0, 0, None, 0, 0, None) == R2L_EINVAL
    assert 'r2l_train_act_backward' in err()
    assert L.r2l_train_act_backward(p, 4, p, 4, None, 0, 1, 4, 9, 1.0, q, 4, None, 0, 0, None, 0, 0, None) == R2L_EINVAL
    assert L.r2l_train_act_backward(p, 4, p, 4, None, 0, 1, 4, 1, 1.0, q, 3, None, 0, 0, None, 0, 0, None) == R2L_EINVAL
    assert L.r2l_train_grad_input(None, 4, 1, p, 4, 4, q, 4, 0, None) == R2L_EINVAL and 'r2l_train_grad_input' in err()
    assert L.r2l_train_grad_input(p, 4, 1, p, 4, 8, q, 4, 0, None) == R2L_EINVAL                                 # ldgx < in_dim
    assert L.r2l_train_grad_input(q, 4, 2, p, 4, 4, q, 4, 0, None) == R2L_EINVAL and 'overlap' in err()
    assert L.r2l_train_grad_weight(p, 4, p, 4, 1, 4, 4, None, None, q, 1 << 20, None) == R2L_EINVAL and 'r2l_train_grad_weight' in err()
    assert L.r2l_train_grad_weight(p, 4, p, 4, 600, 4, 4, q, q, q, 39, None) == R2L_EINVAL and 'workspace' in err()   # 2 slabs x 20 floats
    assert L.r2l_train_grad_weight(p, 4, p, 4, 600, 4, 4, q, q, None, 0, None) == R2L_EINVAL
    assert L.r2l_train_mse_loss(None, p, 1, 1, q, None, q, q, 1, None) == R2L_EINVAL and 'r2l_train_mse_loss' in err()
    assert L.r2l_train_mse_loss(p, p, 300, 1, q, None, q, q, 1, None) == R2L_EINVAL                               # 2 partial sums needed
    assert L.r2l_train_adam(None, p, p, p, 4, 1e-3, 1, None) == R2L_EINVAL and 'r2l_train_adam' in err()
    assert L.r2l_train_adam(p, p, p, p, 4, 1e-3, 0, None) == R2L_EINVAL                                           # steps count from 1
    assert L.r2l_train_adam(p, p, p, p, 4, float('nan'), 1, None) == R2L_EINVAL
    assert L.r2l_train_jitter_z(None, p, 1, 16, q, None) == R2L_EINVAL and 'r2l_train_jitter_z' in err()
    assert L.r2l_train_jitter_z(p, p, 1, 0, q, None) == R2L_EINVAL
    # the slab count of the weight-gradient reduction is a function of n alone
    assert [L.r2l_train_grad_weight_slabs(n) for n in (-1, 0, 1, 512, 513, 4133, 8192, 98304, 10 ** 6)] == [0, 0, 1, 1, 2, 9, 16, 128, 128]


def _fake_trainer(T, plan):
    """An R2LTrainer's state handling over host buffers (the constructor wants a device; the state-dict code does not)."""
    tr = object.__new__(T.R2LTrainer)
    tr.plan = plan
    tr._set_layout([(p['key'], p['in_dim'], p['out_dim']) for p in plan])
    tr._param, tr._grad, tr._m, tr._v = (torch.zeros(tr.n_param) for _ in range(4))
    tr.p, tr.g, tr.exp_avg, tr.exp_avg_sq = (tr._views(b) for b in (tr._param, tr._grad, tr._m, tr._v))
    return tr


def test_optimizer_state_dict_round_trips_through_torch_adam(pkg):
    from efficient_nerf_amd import train as T
    from efficient_nerf_amd.generic import v3_2_plan
    plan = v3_2_plan(6, 8, 12, 3, '', 'relu', True, dict(body_arch='resmlp', n_learnable=2))
    tr = _fake_trainer(T, plan)
    assert tr.optimizer_state_dict()['state'] == {}                         # before the first step, as torch's
    g = torch.Generator().manual_seed(1)
    tr._m.copy_(torch.randn(tr.n_param, generator=g))
    tr._v.copy_(torch.rand(tr.n_param, generator=g))
    tr.t, tr.lr = 7, 3e-4
    osd = tr.optimizer_state_dict()
    params = [torch.nn.Parameter(torch.zeros(shape)) for _, _, shape in tr._slices.values()]       # model.parameters() order
    opt = torch.optim.Adam(params, lr=1.0, betas=(0.9, 0.999))
    opt.load_state_dict(osd)
    assert opt.param_groups[0]['lr'] == 3e-4
    for prm, k in zip(params, tr._slices):
        st = opt.state[prm]
        assert float(st['step']) == 7 and torch.equal(st['exp_avg'], tr.exp_avg[k]) and torch.equal(st['exp_avg_sq'], tr.exp_avg_sq[k])
    for prm in params:                                                      # torch takes a step from that state ...
        prm.grad = torch.randn(prm.shape, generator=g)
    opt.step()
    tr2 = _fake_trainer(T, plan)                                            # ... and its state loads back
    tr2.load_optimizer_state_dict(opt.state_dict())
    assert tr2.t == 8 and tr2.lr == 3e-4
    for prm, k in zip(params, tr2._slices):
        assert torch.equal(tr2.exp_avg[k], opt.state[prm]['exp_avg']) and torch.equal(tr2.exp_avg_sq[k], opt.state[prm]['exp_avg_sq'])
    # an older torch writes `step` as a Python int
    old = opt.state_dict()
    for st in old['state'].values():
        st['step'] = 8
    assert _fake_trainer(T, plan).load_optimizer_state_dict(old).t == 8
    bad = opt.state_dict()
    bad['param_groups'][0]['betas'] = (0.5, 0.999)
    with pytest.raises(T.R2LError):
        _fake_trainer(T, plan).load_optimizer_state_dict(bad)
