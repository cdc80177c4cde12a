"""CPU: LPIPS's host side: metrics.load_lpips_weights on both state_dict layouts, the --test_lpips / --lpips_weights / --lpips_net
flags and their refusals, the argument checks of r2l_lpips and r2l_lpips_workspace_floats (before any device is looked for)."""
import ctypes as C
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONVS = ((64, 3, 11), (192, 64, 5), (384, 192, 3), (256, 384, 3), (256, 256, 3))
SLICES = ('slice1.0', 'slice2.3', 'slice3.6', 'slice4.8', 'slice5.10')
FEATURES = ('features.0', 'features.3', 'features.6', 'features.8', 'features.10')
BASE = ['--model_name', 'R2L', '--render_only', '--pretrained_ckpt', 'x.tar']


def seeded_weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    w = [torch.randn(o, i, k, k, generator=g) * (2 / (i * k * k)) ** .5 for o, i, k in CONVS]
    b = [torch.rand(o, generator=g) * .2 - .1 for o, _, _ in CONVS]
    lin = [torch.rand(o, generator=g) for o, _, _ in CONVS]
    return w + b + lin


def lpips_state_dict(t, lin_key='lin{k}.model.1.weight', prefix=''):
    sd = {f'{prefix}net.{s}.weight': t[k] for k, s in enumerate(SLICES)}
    sd.update({f'{prefix}net.{s}.bias': t[5 + k] for k, s in enumerate(SLICES)})
    sd.update({prefix + lin_key.format(k=k): t[10 + k].view(1, -1, 1, 1) for k in range(5)})
    sd[prefix + 'scaling_layer.shift'] = torch.tensor([-.030, -.088, -.188]).view(1, 3, 1, 1)
    return sd


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('lpips_weights')
    t = seeded_weights()
    paths = {}

    def save(name, sd):
        paths[name] = str(d / name)
        torch.save(sd, paths[name])

    save('one.pth', lpips_state_dict(t))
    save('lins.pth', lpips_state_dict(t, lin_key='lins.{k}.model.1.weight'))
    save('module.pth', lpips_state_dict(t, prefix='module.'))
    alex = {f'{s}.weight': t[k] for k, s in enumerate(FEATURES)}
    alex.update({f'{s}.bias': t[5 + k] for k, s in enumerate(FEATURES)})
    alex.update({'classifier.1.weight': torch.zeros(8, 16), 'classifier.1.bias': torch.zeros(8)})
    save('alexnet.pth', alex)
    save('alex_lin.pth', {f'lin{k}.model.1.weight': t[10 + k].view(1, -1, 1, 1) for k in range(5)})
    bad = lpips_state_dict(t)
    bad['net.slice2.3.weight'] = torch.zeros(192, 64, 3, 3)
    save('wrong_shape.pth', bad)
    short = lpips_state_dict(t)
    del short['lin3.model.1.weight']
    save('missing.pth', short)
    with open(d / 'garbage.pth', 'wb') as fp:
        fp.write(b'not a checkpoint')
    paths['garbage.pth'] = str(d / 'garbage.pth')
    return t, paths


def test_both_layouts_load_to_the_same_15_tensors(pkg, files):
    from efficient_nerf_amd import metrics
    t, paths = files
    for spec in (paths['one.pth'], paths['lins.pth'], paths['module.pth'], paths['alexnet.pth'] + ':' + paths['alex_lin.pth'],
                 paths['alex_lin.pth'] + ':' + paths['alexnet.pth']):
        got = metrics.load_lpips_weights(spec)
        assert len(got) == 15 and all(g.dtype == torch.float32 and g.is_contiguous() and not g.is_cuda for g in got)
        assert [tuple(g.shape) for g in got] == [tuple(v.shape) for v in t]
        assert all(torch.equal(g, v) for g, v in zip(got, t)), spec


def test_a_wrong_shape_or_a_missing_key_is_one_line(pkg, files):
    from efficient_nerf_amd import metrics, R2LError
    _, paths = files
    with pytest.raises(R2LError, match=r'conv 2 weight \(192, 64, 5, 5\).*slice2\.3\.weight.*is \(192, 64, 3, 3\)') as e:
        metrics.load_lpips_weights(paths['wrong_shape.pth'])
    assert '\n' not in str(e.value) and 'e.g. [' in str(e.value)
    with pytest.raises(R2LError, match=r'lin 3 weight \(1, 256, 1, 1\).*lin3\.model\.1\.weight or lins\.3\.model\.1\.weight, no such key') as e:
        metrics.load_lpips_weights(paths['missing.pth'])
    assert '\n' not in str(e.value)
    with pytest.raises(R2LError, match='lin 0 weight'):                  # the trunk alone: the lin layers are the other file's
        metrics.load_lpips_weights(paths['alexnet.pth'])
    with pytest.raises(R2LError, match='cannot read') as e:
        metrics.load_lpips_weights(paths['garbage.pth'])
    assert '\n' not in str(e.value)
    with pytest.raises(R2LError, match='cannot read'):
        metrics.load_lpips_weights(os.path.join(os.path.dirname(paths['one.pth']), 'not_there.pth'))


def test_flags_parse_and_default_to_off(pkg):
    from efficient_nerf_amd.frontend import parse_args
    from efficient_nerf_amd.metrics import lpips_weights_from_args
    args = parse_args(BASE)
    assert args.test_lpips is False and args.lpips_weights == '' and args.lpips_net == 'alex'
    assert lpips_weights_from_args(args) is None
    assert lpips_weights_from_args(parse_args(BASE + ['--lpips_net', 'vgg', '--lpips_weights', 'x.pth'])) is None      # nothing is asked for
    args = parse_args(BASE + ['--test_lpips', '--lpips_weights', 'a.pth:b.pth'])
    assert args.test_lpips is True and args.lpips_weights == 'a.pth:b.pth'


def test_the_three_refusals_come_before_a_device(pkg, files, monkeypatch):
    """--test_lpips without --lpips_weights, with an unreadable or mismatched file, with another trunk: one line each, from main()
    and from train(), before anything initialises a device"""
    from efficient_nerf_amd import frontend, train as T
    _, paths = files

    def no_device(*a, **k):
        raise AssertionError('a device was touched before the refusal')
    monkeypatch.setattr(torch.cuda, 'set_device', no_device)
    monkeypatch.setattr(torch.cuda, 'current_device', no_device)
    from efficient_nerf_amd import dist as D
    monkeypatch.setattr(D, 'init', no_device)
    training = ['--model_name', 'R2L', '--data_mode', 'rays', '--datadir_kd', 'nowhere']
    for extra, what in ((['--test_lpips'], 'needs --lpips_weights'),
                        (['--test_lpips', '--lpips_weights', paths['garbage.pth']], 'cannot read'),
                        (['--test_lpips', '--lpips_weights', paths['wrong_shape.pth']], r'conv 2 weight'),
                        (['--test_lpips', '--lpips_weights', paths['one.pth'], '--lpips_net', 'vgg'], '--lpips_net vgg')):
        for run in (lambda: frontend.main(BASE + extra), lambda: frontend.main(training + extra),
                    lambda: T.train(frontend.parse_args(training + extra), log=lambda *a: None)):
            with pytest.raises(SystemExit, match=what) as e:
                run()
            assert isinstance(e.value.code, str) and '\n' not in e.value.code


def test_lpips_class_refuses_what_the_kernels_do_not_take(pkg):
    from efficient_nerf_amd import metrics
    with pytest.raises(ValueError, match='15 tensors'):
        metrics.LPIPS(seeded_weights()[:14])
    bad = seeded_weights()
    bad[12] = bad[12][:-1]
    with pytest.raises(ValueError, match='15 tensors'):
        metrics.LPIPS(bad)
    m = metrics.LPIPS.__new__(metrics.LPIPS)           # the argument checks of a call need no context
    m._ctx, m.device = None, torch.device('cpu')
    with pytest.raises(ValueError, match='one shape'):
        m(torch.zeros(1, 40, 40, 3), torch.zeros(1, 40, 41, 3))
    with pytest.raises(ValueError, match='GPU'):
        m(torch.zeros(1, 40, 40, 3), torch.zeros(1, 40, 40, 3))


def test_lpips_checks_its_arguments(pkg, built_lib):
    """R2L_EINVAL with a message on bad sizes, NULL pointers or a short workspace, before any device is looked for"""
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    err = lambda: L.r2l_last_error().decode()
    ctx, p, q, ws = C.c_void_p(0x1000), C.c_void_p(0x2000), C.c_void_p(0x100000), C.c_void_p(0x200000)
    ident = (0., 1., 0.) * 2
    need = L.r2l_lpips_workspace_floats(31, 31)
    # 7 x 7, 3 x 3 and 1 x 1 feature maps of both images, and the largest patch matrix (conv 1's: 49 rows of 363 per image)
    assert need >= 2 * 49 * 64 + 2 * 9 * (64 + 192) + 2 * (192 + 384 + 256 + 256) + 2 * 49 * 363
    assert L.r2l_lpips_workspace_floats(400, 400) > need and L.r2l_lpips_workspace_floats(37, 50) > need
    for H, W in ((30, 31), (31, 30), (0, 64), (64, 32769)):
        assert L.r2l_lpips_workspace_floats(H, W) == -1 and 'r2l_lpips_workspace_floats' in err() and f'H={H} W={W}' in err() and '31' in err()
        assert L.r2l_lpips(ctx, p, p, 1, H, W, *ident, q, None, ws, 1 << 40, None) == -1 and f'H={H} W={W}' in err()
    f = L.r2l_lpips
    assert f(None, p, p, 1, 31, 31, *ident, q, None, ws, need, None) == -1 and 'context is NULL' in err()
    assert f(ctx, None, p, 1, 31, 31, *ident, q, None, ws, need, None) == -1 and 'r2l_lpips' in err() and 'NULL' in err()
    assert f(ctx, p, None, 1, 31, 31, *ident, q, None, ws, need, None) == -1 and 'NULL' in err()
    assert f(ctx, p, p, 1, 31, 31, *ident, None, None, ws, need, None) == -1 and 'NULL' in err()
    assert f(ctx, p, p, 1, 31, 31, *ident, q, None, None, need, None) == -1 and 'NULL' in err()
    assert f(ctx, p, p, -1, 31, 31, *ident, q, None, ws, need, None) == -1 and 'n_img=-1' in err()
    assert f(ctx, p, p, 1, 31, 31, *ident, q, None, ws, need - 1, None) == -1 and f'needs {need}' in err()
    assert f(ctx, p, p, 1, 31, 31, *ident, q, None, C.c_void_p(0x200002), need, None) == -1 and 'aligned' in err()
    assert f(None, None, None, 0, 31, 31, *ident, None, None, None, 0, None) == 0          # n_img = 0: a no-op, whatever the pointers
    assert f(None, None, None, 0, 30, 31, *ident, None, None, None, 0, None) == -1         # ... but not whatever the sizes
    out = C.c_void_p()
    assert L.r2l_lpips_create(C.byref(out), None, 15) == -1 and 'r2l_lpips_create' in err()
    arr = (C.c_void_p * 15)(*[C.c_void_p(0x1000)] * 15)
    assert L.r2l_lpips_create(C.byref(out), arr, 14) == -1 and '14 tensors' in err()
    arr[7] = None
    assert L.r2l_lpips_create(C.byref(out), arr, 15) == -1 and 'tensor 7 is NULL' in err()
    L.r2l_lpips_destroy(None)
