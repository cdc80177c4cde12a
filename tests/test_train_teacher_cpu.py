"""CPU: the parts of teacher training that need no device -- the command line and its defaults, the crop and the pixel selection of
the image loop, the parameter order, the checkpoint's keys, the refusals, and the argument checks of the new C-ABI entry point."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGO = ['--config', os.path.join(ROOT, 'configs', 'lego.txt')]


def test_flag_defaults_are_the_references(pkg):
    """option.py of the reference: i_testset 2000, i_video 10000, select_pixel_mode rand_pixel, precrop_iters 0, precrop_frac 0.5,
    N_rand 4096, lrate 5e-4, lrate_decay 250, perturb 1, raw_noise_std 0, i_weights 10000, i_print 100, testskip 8"""
    from efficient_nerf_amd import frontend as fe
    d = fe.parse_args([])
    assert (d.i_testset, d.i_video, d.select_pixel_mode, d.precrop_iters, d.precrop_frac, d.N_rand, d.lrate, d.lrate_decay, d.perturb,
            d.raw_noise_std, d.i_weights, d.i_print, d.testskip, d.no_batching, d.N_iters) == \
        (2000, 10000, 'rand_pixel', 0, .5, 4096, 5e-4, 250, 1., 0., 10000, 100, 8, False, 200000)
    a = fe.parse_args(LEGO)
    assert (a.no_batching, a.use_viewdirs, a.white_bkgd, a.lrate_decay, a.N_samples, a.N_importance, a.N_rand, a.precrop_iters,
            a.precrop_frac, a.half_res, a.dataset_type) == (True, True, True, 500, 64, 128, 1024, 500, .5, True, 'blender')
    with pytest.raises(SystemExit):
        fe.parse_args(['--select_pixel_mode', 'other'])


def test_crop_and_pixel_selection_follow_the_reference_stream(pkg):
    """main.py:1270-1291 with get_selected_coords(..., 'rand_pixel'): coords is the meshgrid of linspace(H//2 - dH, H//2 + dH - 1,
    2 dH) x linspace(...) (or the whole image), flattened row-major and indexed by ONE np.random.choice(h * w, N_rand,
    replace=False) of the global stream"""
    from efficient_nerf_amd.train_teacher import crop_bounds, select_coords
    for H, W, frac, n_rand in ((400, 400, .5, 1024), (37, 52, .5, 100), (64, 48, .3, 50)):
        dH, dW = int(H // 2 * frac), int(W // 2 * frac)
        for cropped in (True, False):
            if cropped:
                coords = torch.stack(torch.meshgrid(torch.linspace(H // 2 - dH, H // 2 + dH - 1, 2 * dH),
                                                    torch.linspace(W // 2 - dW, W // 2 + dW - 1, 2 * dW), indexing='ij'), -1)
            else:
                coords = torch.stack(torch.meshgrid(torch.linspace(0, H - 1, H), torch.linspace(0, W - 1, W), indexing='ij'), -1)
            np.random.seed(5)
            ix = np.random.choice(coords.shape[0] * coords.shape[1], size=[n_rand], replace=False)
            want = coords.long().view(-1, 2)[ix]
            follow = np.random.rand()
            np.random.seed(5)
            rows, cols = select_coords(H, W, n_rand, crop_bounds(H, W, frac) if cropped else None)
            assert np.random.rand() == follow                                  # the stream is where the reference leaves it
            assert np.array_equal(rows, want[:, 0].numpy()) and np.array_equal(cols, want[:, 1].numpy())
            assert len(set(zip(rows.tolist(), cols.tolist()))) == n_rand
    assert crop_bounds(400, 400, .5) == (100, 200, 100, 200)
    from efficient_nerf_amd import R2LError
    with pytest.raises(R2LError):
        select_coords(32, 32, 1024, crop_bounds(32, 32, .5))


def test_parameter_order_is_the_module_creation_order(pkg):
    from efficient_nerf_amd.train_teacher import reference_order
    from oracle import r2l_oracle as O
    for D, W, ic, icv, och, vd in ((8, 256, 63, 27, 5, True), (4, 128, 27, 15, 4, True), (6, 64, 63, 0, 5, False), (2, 32, 3, 3, 5, True)):
        plan = reference_order(D, W, ic, icv, och, vd)
        names = [f'{k}.{kind}' for k, _, _ in plan for kind in ('weight', 'bias')]
        sd = O.make_nerf_state(0, D, W, ic, icv, och, (4,), vd)
        assert names == list(sd)
        assert all(tuple(sd[k + '.weight'].shape) == (o, i) and tuple(sd[k + '.bias'].shape) == (o,) for k, i, o in plan)
    keys = [k for k, _, _ in reference_order(8, 256, 63, 27, 5, True)]
    assert keys[8:] == ['views_linears.0', 'feature_linear', 'alpha_linear', 'rgb_linear']
    assert [k for k, _, _ in reference_order(8, 256, 63, 0, 5, False)][8:] == ['views_linears.0', 'output_linear']


class _FakeTeacher:
    """what save_train_checkpoint reads of a NeRFTrainer"""

    def __init__(self, fine=True):
        self.fine = fine

    def state_dicts(self):
        return {'pts_linears.0.weight': torch.ones(2, 3)}, ({'pts_linears.0.weight': torch.zeros(2, 3)} if self.fine else None)

    def optimizer_state_dict(self):
        return {'state': {}, 'param_groups': [{'lr': 1e-3, 'params': [0, 1]}]}


def test_checkpoint_keys(pkg, tmp_path):
    """main.py:1516-1537: network_fine_state_dict beside network_fn_state_dict when there is a fine network; loads through the
    front end's reader"""
    from efficient_nerf_amd import frontend as fe
    from efficient_nerf_amd.train import save_train_checkpoint
    p = save_train_checkpoint(str(tmp_path / 'ckpt.tar'), _FakeTeacher(True), 7, 21.5, 5)
    ck = fe.load_checkpoint(p)
    assert set(ck) == {'global_step', 'best_psnr', 'best_psnr_step', 'network_fn_state_dict', 'network_fine_state_dict', 'optimizer_state_dict'}
    assert (ck['global_step'], ck['best_psnr'], ck['best_psnr_step']) == (7, 21.5, 5)
    assert ck['network_fn_state_dict']['pts_linears.0.weight'].sum() == 6 and not ck['network_fine_state_dict']['pts_linears.0.weight'].any()
    ck = fe.load_checkpoint(save_train_checkpoint(str(tmp_path / 'c.tar'), _FakeTeacher(False), 1))
    assert 'network_fine_state_dict' not in ck


@pytest.mark.parametrize('extra,line', [
    (['--use_batching_stand_in'], 'use_batching'),
    (['--dataset_type', 'llff'], '--dataset_type llff: teacher training is built for Blender scenes'),
    (['--select_pixel_mode', 'rand_patch'], '--select_pixel_mode rand_patch'),
    (['--i_video', '50', '--N_iters', '100'], '--i_video 50 falls inside this run'),
    (['--datadir_kd', 'DIR'], '--datadir_kd with --data_mode images'),
    (['--data_mode', 'rays'], '--data_mode rays: the teacher trains on images'),
    (['--model_name', 'R2L'], '--model_name R2L: train_teacher.py trains --model_name nerf'),
    (['--render_only'], 'train_teacher.py trains; render with main.py'),
    (['--i_testset', '-5'], '--i_testset -5: a positive interval, or 0 for no test renders'),
])
def test_each_refused_mode_exits_with_its_line(pkg, tmp_path, extra, line):
    from efficient_nerf_amd import train_teacher as TT
    argv = LEGO + ['--i_video', '1000000'] + extra
    if extra == ['--use_batching_stand_in']:          # use_batching is the absence of no_batching: a config without that line
        cfg = tmp_path / 'batching.txt'
        cfg.write_text('dataset_type = blender\nuse_viewdirs = True\n')
        argv = ['--config', str(cfg), '--i_video', '1000000']
    with pytest.raises(SystemExit) as e:
        TT.main(argv)
    assert line in str(e.value) and '\n' not in str(e.value)


def test_main_py_keeps_refusing_and_points_here(pkg):
    from efficient_nerf_amd import frontend as fe
    with pytest.raises(SystemExit) as e:
        fe.main(['--model_name', 'nerf'] + LEGO)
    assert 'teacher training is not built' in str(e.value) and 'train_teacher.py' in str(e.value)


def test_scan_backward_checks_its_arguments(pkg, built_lib):
    """R2L_EINVAL with a message on NULL or bad arguments, before any device is looked for"""
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    err = lambda: L.r2l_last_error().decode()
    p, q = C.c_void_p(0x1000), C.c_void_p(0x100000)
    f = L.nerf_train_raw2outputs_backward
    assert f(None, p, p, None, 4, 64, 1, p, q, None) == -1 and 'nerf_train_raw2outputs_backward' in err()
    assert f(p, p, p, None, 4, 64, 1, p, None, None) == -1
    assert f(p, p, p, None, -1, 64, 1, p, q, None) == -1
    assert f(p, p, p, None, 4, 0, 1, p, q, None) == -1 and 'S=0' in err()
    assert f(p, p, p, None, 4, 64, 1, p, C.c_void_p(0x100004), None) == -1 and 'aligned' in err()
    assert f(p, p, p, None, 4, 64, 1, p, p, None) == -1 and 'must not be raw' in err()


def test_frozen_parameters_have_no_optimizer_state(pkg):
    """FlatAdam: a parameter that never receives a gradient (views_linears.0 without view directions) has no entry in the saved
    state, as torch.optim.Adam keeps none for a .grad of None; a state with or without such entries loads"""
    from efficient_nerf_amd import train as T
    tr = object.__new__(T.FlatAdam)
    shapes = {'a.weight': (3, 2), 'views_linears.0.weight': (2, 2), 'b.bias': (3,)}
    tr._slices, off = T.OrderedDict(), 0
    for k, shape in shapes.items():
        tr._slices[k] = (off, int(np.prod(shape)), shape)
        off += int(np.prod(shape))
    tr._frozen = frozenset(['views_linears.0.weight'])
    tr.n_param, tr.t, tr.lr = off, 4, 1e-3
    tr._param, tr._grad, tr._m, tr._v = (torch.rand(off) for _ in range(4))
    tr.p, tr.g, tr.exp_avg, tr.exp_avg_sq = (tr._views(b) for b in (tr._param, tr._grad, tr._m, tr._v))
    osd = tr.optimizer_state_dict()
    assert sorted(osd['state']) == [0, 2]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes.values()]
    opt = torch.optim.Adam(params, lr=1.0)
    opt.load_state_dict(osd)
    params[0].grad, params[2].grad = torch.ones(3, 2), torch.ones(3)
    opt.step()
    assert not params[1].any() and sorted(opt.state_dict()['state']) == [0, 2]
    tr.load_optimizer_state_dict(opt.state_dict())
    assert tr.t == 5 and not tr.exp_avg['views_linears.0.weight'].any()
    assert torch.equal(tr.exp_avg['a.weight'], opt.state[params[0]]['exp_avg'])
