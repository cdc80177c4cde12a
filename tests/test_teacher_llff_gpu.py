"""GPU: teacher training on LLFF scenes -- nerf_train_batch_rays (csrc/nerf_train.hip) against the launches it replaces and the
reference's recorded bank rows, `viewdirs=` in NeRFTrainer, a short run through RayBatches, and the command line.

The scene is tests/golden/llff/scene: 10 views of 30 x 40, focal 37.5; with every 8th view held out 8 views train: 9,600 rays, nine
batches of 1,024 and one of 384 per epoch.  Yardsticks and bands of the whole-step case are tests/test_train_teacher_gpu.py's."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import test_train_teacher_gpu as TG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, 'tests', 'golden', 'llff', 'scene')
FILL = -777.
PAD = 64
WINDOWS = [(1, 0), (384, 9216), (1024, 0), (1024, 2049)]       # (rows, offset): one ray; the epoch's short last batch; full; odd offset


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope='module')
def L(pkg, built_lib):
    from efficient_nerf_amd import _lib
    return _lib.lib()


@pytest.fixture(scope='module')
def data(pkg):
    """the 8 training views on the device, and one permutation of their 9,600 rays"""
    from efficient_nerf_amd import llff
    from efficient_nerf_amd.train_teacher import llff_split_and_bounds
    scene = llff.load_scene(SCENE, 8)
    i_train = llff_split_and_bounds(scene, 8, False)[0]
    H, W, focal = scene.hwf
    n = len(i_train) * H * W
    assert (len(i_train), H, W, n) == (8, 30, 40, 9600)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3))
    return dict(bytes=torch.from_numpy(scene.bytes[i_train]).cuda().contiguous(), n_img=len(i_train), H=H, W=W, focal=focal, n=n,
                poses=torch.from_numpy(scene.poses[i_train][:, :3, :4].copy()).cuda().contiguous(), perm=perm.cuda(), scene=scene, i_train=i_train)


def _batch(L, d, order, ndc, with_viewdirs=True, rows=None):
    """nerf_train_batch_rays into the middle of four buffers filled with FILL: ([rays_o, rays_d, viewdirs, target], the margins)"""
    rows = order.shape[0] if rows is None else rows
    bufs = [torch.full((PAD + 3 * max(rows, 1) + PAD,), FILL, device='cuda') for _ in range(4)]
    outs = [b[PAD:PAD + 3 * rows] for b in bufs]
    ptrs = [C.c_void_p(b.data_ptr() + 4 * PAD) for b in bufs]
    if not with_viewdirs:
        ptrs[2] = None
    rc = L.nerf_train_batch_rays(_p(d['bytes']), d['n_img'], d['H'], d['W'], _p(d['poses']), d['focal'], _p(order), rows, ndc, 1., ptrs[0],
                                 ptrs[1], ptrs[2], ptrs[3], _stream())
    assert rc == 0, L.r2l_last_error().decode()
    torch.cuda.synchronize()
    margins = torch.cat([torch.cat([b[:PAD], b[PAD + 3 * rows:]]) for b in bufs])
    return [o.view(rows, 3).clone() for o in outs], margins


def _convert(L, d, order):
    """r2l_rays_from_images on the same window: [rows, 9]"""
    rows = order.shape[0]
    out = torch.empty((rows, 9), device='cuda')
    rc = L.r2l_rays_from_images(_p(d['bytes']), d['n_img'], d['H'], d['W'], 3, _p(d['poses']), d['focal'], 0, _p(order), rows, _p(out), _stream())
    assert rc == 0, L.r2l_last_error().decode()
    return out


@pytest.mark.parametrize('rows,offset', WINDOWS)
def test_batch_rays_equal_the_launches_they_replace(L, data, rows, offset):
    """ndc = 0: rays_o, rays_d and target are r2l_rays_from_images' [rows, 9] bit for bit; ndc = 1: rays_o and rays_d are
    nerf_ndc_rays of those bit for bit; viewdirs is the same in both modes and within 5e-7 of the float64 normalisation of the
    kernel's own world directions; nothing is written beside the rows; viewdirs_dev = NULL leaves the other three as they are"""
    from efficient_nerf_amd import ndc_rays
    order = data['perm'][offset:offset + rows]
    assert order.shape[0] == rows and order.data_ptr() % 8 == 0
    (o0, d0, v0, t0), m0 = _batch(L, data, order, 0)
    (o1, d1, v1, t1), m1 = _batch(L, data, order, 1)
    want = _convert(L, data, order)
    assert torch.equal(o0, want[:, 0:3]) and torch.equal(d0, want[:, 3:6]) and torch.equal(t0, want[:, 6:9])
    no, nd = ndc_rays(data['H'], data['W'], data['focal'], 1., o0, d0)
    assert torch.equal(o1, no) and torch.equal(d1, nd) and torch.equal(t1, t0)
    assert torch.equal(v0, v1)
    d64 = d0.double()
    gap = float((v0.double() - d64 / d64.norm(dim=-1, keepdim=True)).abs().max())
    print(f'rows {rows} offset {offset}: max |viewdirs - float64 normalisation| = {gap:.2e}')
    assert gap <= 5e-7
    assert torch.isfinite(torch.cat([o0, d0, v0, t0, o1, d1])).all()
    assert bool((m0 == FILL).all()) and bool((m1 == FILL).all())
    for ndc, ref in ((0, (o0, d0, t0)), (1, (o1, d1, t1))):
        (o, d_, v, t), m = _batch(L, data, order, ndc, with_viewdirs=False)
        assert torch.equal(o, ref[0]) and torch.equal(d_, ref[1]) and torch.equal(t, ref[2])
        assert bool((v == FILL).all()) and bool((m == FILL).all())


def test_batch_rays_against_the_references_recorded_rows(L, data, golden_dir):
    """256 rows of the reference's bank (get_rays_np beside the images), its normalisation and its ndc_rays of them: all four
    outputs within 5e-7, the world-space origins bit-equal"""
    g = np.load(os.path.join(golden_dir, 'llff_teacher', 'rows.npz'))
    order = torch.from_numpy(g['rows']).cuda()
    (o0, d0, v0, t0), _ = _batch(L, data, order, 0)
    (o1, d1, v1, t1), _ = _batch(L, data, order, 1)
    dev = lambda k: torch.from_numpy(g[k]).cuda()
    assert torch.equal(o0, dev('rays_o'))
    gaps = {}
    for name, got, key in (('rays_d', d0, 'rays_d'), ('viewdirs', v0, 'viewdirs'), ('target', t0, 'target'), ('ndc rays_o', o1, 'ndc_o'),
                           ('ndc rays_d', d1, 'ndc_d'), ('ndc viewdirs', v1, 'viewdirs'), ('ndc target', t1, 'target')):
        gaps[name] = float((got.double() - dev(key).double()).abs().max())
    print('max gap from the recorded rows: ' + ', '.join(f'{k} {v:.2e}' for k, v in gaps.items()))
    assert all(v <= 5e-7 for v in gaps.values()), gaps


def test_batch_rays_out_of_range_index_and_empty_batch(L, data):
    """an index outside [0, n) gives NaN in that ray's four rows and leaves its neighbours' bits; rows = 0 touches nothing"""
    order = data['perm'][:300].clone()
    clean, _ = _batch(L, data, order, 1)
    bad = {0: -1, 63: data['n'], 64: 1 << 40, 299: -(1 << 33)}
    for k, v in bad.items():
        order[k] = v
    got, margins = _batch(L, data, order, 1)
    keep = torch.ones(300, dtype=torch.bool, device='cuda')
    keep[list(bad)] = False
    for a, b in zip(got, clean):
        assert torch.isnan(a[~keep]).all() and torch.equal(a[keep], b[keep])
    assert bool((margins == FILL).all())
    for ndc in (0, 1):
        outs, margins = _batch(L, data, data['perm'][:1], ndc, rows=0)
        assert bool((margins == FILL).all()) and all(o.numel() == 0 for o in outs)
    assert L.nerf_train_batch_rays(_p(data['bytes']), 8, 30, 40, _p(data['poses']), 37.5, None, 0, 1, 1., None, None, None, None, _stream()) == 0


# ---- viewdirs= in the trainer --------------------------------------------------------------------------------------------------
def _kernel_rays(L, data, rows, ndc, offset=0):
    (o, d, v, t), _ = _batch(L, data, data['perm'][offset:offset + rows], ndc)
    return o.contiguous(), d.contiguous(), v.contiguous(), t.contiguous()


def test_explicit_viewdirs_change_no_bit(pkg):
    """the smallest variant of tests/test_train_teacher_gpu.py: passing viewdirs = rd / ||rd|| gives the loss and every gradient
    bit-equal to the call without it"""
    from efficient_nerf_amd.train_teacher import NeRFTrainer
    from oracle import r2l_oracle as O
    n = 300
    tr = NeRFTrainer(max_rays=n, **TG._cfg())
    tr.load_state_dicts(*TG._states(O, tr, 31))
    g = torch.Generator().manual_seed(1031)
    ro, rd, tgt = TG._rays(n, 31, 'cuda')
    t_rand, u = torch.rand(n, tr.N_samples, generator=g).cuda(), torch.rand(n, tr.N_importance, generator=g).cuda()
    noise = tuple(torch.randn(n, net.S, generator=g).cuda() for net in tr.nets)
    loss_a = tr.forward_backward(ro, rd, tgt, perturb=1., t_rand=t_rand, u=u, noise=noise).clone()
    grads_a = tr.grads()
    vd = rd / torch.norm(rd, dim=-1, keepdim=True)
    loss_b = tr.forward_backward(ro, rd, tgt, perturb=1., t_rand=t_rand, u=u, noise=noise, viewdirs=vd).clone()
    grads_b = tr.grads()
    assert torch.equal(loss_a, loss_b) and float(loss_a) > 0
    assert all(torch.equal(a[k], b[k]) for a, b in zip(grads_a, grads_b) for k in a)
    loss_c = tr.forward_backward(ro, rd, tgt, perturb=1., t_rand=t_rand, u=u, noise=noise, viewdirs=-vd)     # ... and they are read
    assert not torch.equal(loss_a, loss_c)
    from efficient_nerf_amd import R2LError
    with pytest.raises(R2LError):
        tr.forward_backward(ro, rd, tgt, viewdirs=vd[:-1])


def test_ndc_inputs_render_as_generic_nerf(L, data, pkg):
    """NDC rays and world view directions from the kernel, perturb = 0, no noise: the trainer's rgb and rgb0 against
    GenericNeRF(ndc=True) on the same world rays and weights.  Bound: 4 x the largest gap the same two paths show on the non-NDC
    call of those rays (measured here), not less than one fp32 spacing at 1"""
    from efficient_nerf_amd.generic import GenericNeRF
    from efficient_nerf_amd.train_teacher import NeRFTrainer
    from oracle import r2l_oracle as O
    n = 300
    cfg = TG._cfg(white_bkgd=False)
    tr = NeRFTrainer(0., 1., max_rays=n, **cfg)
    sds = TG._states(O, tr, 32)
    tr.load_state_dicts(*sds)
    wo, wd, wv, tgt = _kernel_rays(L, data, n, 0)
    no, nd, nv, _ = _kernel_rays(L, data, n, 1)
    gaps = {}
    for ndc, (ro, rd, vd) in ((False, (wo, wd, None)), (True, (no, nd, nv))):
        eng = GenericNeRF(data['H'], data['W'], data['focal'], 0., 1., ndc=ndc, **cfg).load_state_dicts(*sds)
        want = eng.render_rays(wo, wd, extras=True)
        tr.forward_backward(ro, rd, tgt, perturb=0., viewdirs=vd)
        assert torch.isfinite(tr.last['rgb']).all() and torch.isfinite(want['rgb_map']).all()
        gaps[ndc] = max(float((tr.last['rgb'] - want['rgb_map']).abs().max()), float((tr.last['rgb0'] - want['rgb0']).abs().max()))
    bound = max(4 * gaps[False], 2. ** -23)
    print(f'trainer against GenericNeRF, max |rgb| and |rgb0| gap: world rays {gaps[False]:.2e}, NDC {gaps[True]:.2e} (bound {bound:.2e})')
    assert gaps[True] <= bound


def test_whole_step_gradients_with_ndc_inputs_and_noise(L, data, pkg):
    """one whole step on NDC rays with the world view directions and raw_noise_std = 1 against float64 autograd: the HIP gap within
    4 x torch fp32 autograd's (yardstick and band of tests/test_train_teacher_gpu.py); a second run gives the same bits"""
    from efficient_nerf_amd.train_teacher import NeRFTrainer
    from oracle import r2l_oracle as O
    n = 300
    tr = NeRFTrainer(0., 1., max_rays=n, **TG._cfg(white_bkgd=False))
    sds = TG._states(O, tr, 33)
    tr.load_state_dicts(*sds)
    ro, rd, vd, tgt = _kernel_rays(L, data, n, 1, offset=777)
    g = torch.Generator().manual_seed(1033)
    t_rand, u = torch.rand(n, tr.N_samples, generator=g).cuda(), torch.rand(n, tr.N_importance, generator=g).cuda()
    noise = tuple(1. * torch.randn(n, net.S, generator=g).cuda() for net in tr.nets)
    loss = float(tr.forward_backward(ro, rd, tgt, perturb=1., t_rand=t_rand, u=u, noise=noise, viewdirs=vd).item())
    got = [g_ for g_ in tr.grads() if g_ is not None]
    assert torch.equal(tr.last['dirs0'].view(n, tr.N_samples, -1)[:, 0, :3], vd)      # the embedded directions are the given ones
    l64, g64 = TG._yardstick(O, tr, sds, rd, tgt, torch.float64)
    l32, g32 = TG._yardstick(O, tr, sds, rd, tgt, torch.float32)
    assert all(torch.isfinite(v).all() for gn in got for v in gn.values())
    TG._band_check('NDC inputs, raw_noise_std 1', [TG._gaps(got, g64)], [TG._gaps(g32, g64)], [(loss, l32, l64)])
    loss2 = float(tr.forward_backward(ro, rd, tgt, perturb=1., t_rand=t_rand, u=u, noise=noise, viewdirs=vd).item())
    again = [g_ for g_ in tr.grads() if g_ is not None]
    assert loss2 == loss and all(torch.equal(a[k], b[k]) for a, b in zip(got, again) for k in a)


# ---- a short run ---------------------------------------------------------------------------------------------------------------
def test_short_run_through_ray_batches(data, pkg):
    """40 steps on the fixture at N_rand 1024, NDC, raw_noise_std 1: four epochs, each ending on its 384-ray batch and a reshuffle.
    The mean loss of the last 10 steps is below that of the first 10; a second run from the same seeds ends on the same bits"""
    from efficient_nerf_amd.train_teacher import NeRFTrainer, RayBatches
    from oracle import r2l_oracle as O
    scene, i_train = data['scene'], data['i_train']
    tr = NeRFTrainer(0., 1., max_rays=1024, **dict(TG.RUN, white_bkgd=False))
    sds = TG._states(O, tr, 34)

    def run():
        np.random.seed(11)
        torch.manual_seed(12)
        lines = []
        rb = RayBatches(scene.bytes[i_train], scene.poses[i_train], data['focal'], 1024, True, log=lines.append)
        tr.load_state_dicts(*sds)
        tr.load_optimizer_state_dict({'state': {}, 'param_groups': tr.optimizer_state_dict()['param_groups']})
        losses, sizes = [], []
        for _ in range(40):
            ro, rd, vd, tgt = rb.next()
            sizes.append(ro.shape[0])
            loss, _ = tr.step(ro, rd, tgt, 2e-3, perturb=1., raw_noise_std=1., viewdirs=vd)
            losses.append(loss.clone())
        assert sizes == ([1024] * 9 + [384]) * 4 and lines == ['Shuffle data after an epoch!'] * 4
        return torch.cat(losses).cpu(), tr.state_dicts()

    l1, sd1 = run()
    l2, sd2 = run()
    print(f'mean loss of steps 0-9 {float(l1[:10].mean()):.5f}, of steps 30-39 {float(l1[30:].mean()):.5f}')
    assert torch.isfinite(l1).all() and float(l1[30:].mean()) < float(l1[:10].mean())
    assert torch.equal(l1, l2)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(sd1, sd2) for k in a)


# ---- command line --------------------------------------------------------------------------------------------------------------
def test_cli_trains_tests_saves_renders_and_resumes_on_llff(pkg, tmp_path):
    """train_teacher.py with configs/fern.txt as a child process on the fixture; main.py --render_only --render_test on its
    checkpoint; --resume from it.  Each child under its own timeout; a failure starts nothing further."""
    net = ['--N_samples', '16', '--N_importance', '16', '--netwidth', '64']
    base = ['--config', os.path.join(ROOT, 'configs', 'fern.txt'), '--datadir', SCENE, '--basedir', str(tmp_path), '--expname', 'cli'] + net
    train = ['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'train_teacher.py')] + base + [
        '--lrate', '0.002', '--i_print', '5', '--i_weights', '15', '--i_video', '100000']
    out = TG._run(train + ['--N_iters', '30', '--i_testset', '30'], str(tmp_path))
    lines = [ln for ln in out.splitlines() if ln.startswith('[TRAIN] Iter')]
    assert len(lines) == 6, out[-3000:]
    assert all(re.fullmatch(r'\[TRAIN\] Iter \d+ data_time \d+\.\d{4} batch_time \d+\.\d{4} loss \d+\.\d{6} psnr \S+ hist_psnr \S+ LR \d\.\d{10}', ln)
               for ln in lines), lines
    hist = [float(re.search(r'hist_psnr (\S+)', ln).group(1)) for ln in lines]
    assert hist[-1] > hist[0], hist
    assert out.count('Shuffle data after an epoch!') == 3 and 'Center cropping' not in out
    assert 'Loaded llff (10, 30, 40, 3)' in out and '8 train / 2 val / 2 test images' in out and 'near 0.0000 far 1.0000, NDC' in out
    tests = [ln for ln in out.splitlines() if ln.startswith('[TEST] Iter')]
    assert len(tests) == 1 and re.match(r'\[TEST\] Iter 30 TestPSNR \S+ TestPSNRv2 \S+ BestPSNRv2 \S+ \(Iter 30\)', tests[0]), tests
    wdir = tmp_path / 'cli' / 'weights'
    for name in ('ckpt.tar', 'ckpt_best.tar'):
        saved = torch.load(str(wdir / name), map_location='cpu', weights_only=False)
        assert {'network_fn_state_dict', 'network_fine_state_dict', 'optimizer_state_dict', 'global_step', 'best_psnr', 'best_psnr_step'} <= set(saved)
        assert saved['global_step'] == 30 and len(saved['optimizer_state_dict']['state']) == 2 * 24
        assert list(saved['network_fn_state_dict'])[16:18] == ['views_linears.0.weight', 'views_linears.0.bias']
        assert tuple(saved['network_fn_state_dict']['pts_linears.0.weight'].shape) == (64, 63)
    ck = str(wdir / 'ckpt.tar')
    outdir = str(tmp_path / 'render')
    TG._run(['timeout', '-k', '10', '300', sys.executable, os.path.join(ROOT, 'main.py'), '--model_name', 'nerf', '--dataset_type', 'llff',
             '--datadir', SCENE, '--use_viewdirs'] + net + ['--pretrained_ckpt', ck, '--render_only', '--render_test', '--outdir', outdir],
            str(tmp_path))
    rgbs = np.load(os.path.join(outdir, 'rgbs.npy'))
    assert rgbs.shape == (2, 30, 40, 3) and np.isfinite(rgbs).all()
    out = TG._run(train + ['--N_iters', '40', '--i_testset', '1000', '--pretrained_ckpt', ck, '--resume'], str(tmp_path))
    assert 'Resume optimizer successfully.' in out
    its = [int(re.search(r'Iter (\d+)', ln).group(1)) for ln in out.splitlines() if ln.startswith('[TRAIN] Iter')]
    assert its == [35, 40], out[-2000:]
    assert out.count('Shuffle data after an epoch!') == 1                # a fresh epoch from step 31: its tenth batch is step 40
    assert torch.load(ck, map_location='cpu', weights_only=False)['global_step'] == 40
