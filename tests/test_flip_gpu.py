"""GPU: FLIP on the library's kernels (csrc/r2l_flip.hip, efficient-nerf_amd/metrics.py flip) and TestFLIP on the [TEST] lines
behind --test_flip.

The yardstick is tests/golden/flip.npz (make_golden_flip.py): the reference's own utils/flip_loss.py evaluated in float64, with
`band` = L_inf between its float32 and its float64 evaluation of the same case.  A map passes within 4 x band: two independent
float32 evaluations can each sit one band from exact, and the separable summation order gets the other factor of two.  The band a
case is held to is the largest among the plain natural-image cases at its pixels_per_degree (one 5 x 7 case's own band is too lucky
a sample), or its own where that is larger (the rescaled pair, whose dark half is the more sensitive input); white against black,
an input of another kind, is held to its own.  No pixel is excluded.

tests/golden/flip_edges.npz (make_golden_flip_edges.py) holds the same for the edges of the kernels' tiles and radii, EDGES below:
natural pairs at pixels_per_degree 118 (radii 16 and 15, the largest the kernels accept: the column kernel's 64-row LDS tile, the row
kernel's 160-wide rows and the padded tap rows are used to their last element), 5 (radii 1 and 1) and 16 (3 and 2), as one-pixel
strips, a frame smaller than every filter, exact multiples of the 64 x 32 and 128 x 2 tiles and one pixel past them; same rule, the
band the largest among the edge cases at the same pixels_per_degree.  Its last case has one NaN and one +Inf pixel: the map's NaN
set must be the reference's (the 21 x 21 box the dense filters reach from the NaN pixel; the column pass slides eight outputs over
zero-padded taps and 0 * NaN is NaN, so it has to sum such outputs again over their own rows), the finite pixels are held to the
rule, the mean is NaN with and without a map, and the Inf is clamped to 1 as the reference clamps it."""
import ctypes as C
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
NATURAL = (0, 1, 2, 3, 4, 8, 9, 10)          # plain natural-image pairs (make_golden_flip.py); 5 identical, 6 white / black, 7 rescaled
IDENTICAL, WHITE_BLACK, RESCALED = 5, 6, 7
N_CASES = 11
# flip_edges.npz: (pixels_per_degree, (CSF radius, feature radius), (H, W)) of its natural pairs, then the NaN / Inf pair
EDGES = [(118.0, (16, 15), hw) for hw in ((1, 70), (70, 1), (3, 5), (32, 64), (32, 128), (33, 129))] + \
        [(5.0, (1, 1), hw) for hw in ((3, 5), (1, 70), (33, 129))] + [(16.0, (3, 2), hw) for hw in ((70, 1), (32, 64))]
NAN_CASE, NAN_BOX = len(EDGES), (slice(10, 31), slice(20, 41))          # a[20, 30, 1] = NaN at radii (10, 9)


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'flip.npz'))


def _case(golden, k):
    return (torch.tensor(golden[f'a_{k}'].astype(np.float32)).cuda()[None], torch.tensor(golden[f'b_{k}'].astype(np.float32)).cuda()[None],
            float(golden[f'ppd_{k}']), bool(golden[f'rescale_{k}']))


def _band(golden, k):
    if k == WHITE_BLACK:
        return float(golden[f'band_{k}'])
    group = max(float(golden[f'band_{j}']) for j in NATURAL if float(golden[f'ppd_{j}']) == float(golden[f'ppd_{k}']))
    return max(group, float(golden[f'band_{k}']))


@pytest.fixture(scope='module')
def edges(golden_dir):
    return np.load(os.path.join(golden_dir, 'flip_edges.npz'))


def _edge_case(edges, k):
    return (torch.tensor(edges[f'a_{k}'].astype(np.float32)).cuda()[None], torch.tensor(edges[f'b_{k}'].astype(np.float32)).cuda()[None],
            float(edges[f'ppd_{k}']))


def _radii(ppd):
    """the filter radii the library builds its taps for at `ppd`"""
    from efficient_nerf_amd import _lib
    buf, rc, rf = (C.c_float * (7 * 33))(), C.c_int(), C.c_int()
    _lib.check(_lib.lib().r2l_flip_taps(float(ppd), buf, C.byref(rc), C.byref(rf)))
    return rc.value, rf.value


@pytest.mark.parametrize('k', range(N_CASES))
def test_golden_case(pkg, built_lib, golden, k):
    """map and mean of every golden case against the reference's float64 result"""
    from efficient_nerf_amd import metrics
    a, b, ppd, resc = _case(golden, k)
    mean, fmap = metrics.flip(a, b, pixels_per_degree=ppd, rescale=resc, return_map=True)
    want = golden[f'map64_{k}']
    got = fmap[0].cpu().numpy().astype(np.float64)
    assert got.shape == want.shape
    if k == IDENTICAL:
        assert np.all(got == 0.0) and mean == 0.0
        return
    band = _band(golden, k)
    err, err_mean = np.abs(got - want).max(), abs(mean - float(golden[f'mean64_{k}']))
    print(f'case {k} {want.shape} pixels_per_degree {ppd:.2f} rescale {resc}: L_inf {err:.3e} = {err / band:.2f} band ({band:.2e}), mean off by '
          f'{err_mean:.3e} (mean {mean:.6f})')
    assert np.isfinite(got).all()
    assert err <= 4 * band and err_mean <= 4 * band


def _stack_checks(a0, b0, ppd):
    from efficient_nerf_amd import _lib, metrics
    a = torch.cat([a0, b0.flip(1), a0.flip(2) * 0.5], 0).contiguous()
    b = torch.cat([b0, a0.flip(1) * 0.9, b0.flip(2) * 0.5 + 0.1], 0).contiguous()
    n, H, W = a.shape[:3]
    L = _lib.lib()
    need = L.r2l_flip_workspace_floats(H, W, ppd)

    def call(x, y, with_map=True):
        ws = torch.full((need,), float('nan'), device='cuda')
        fmap = torch.full((len(x), H, W), -1., device='cuda') if with_map else None
        means = torch.full((len(x),), -1., device='cuda')
        _lib.check(L.r2l_flip(_lib.dptr(x), _lib.dptr(y), len(x), H, W, 0., 1., 0., 0., 1., 0., ppd, _lib.dptr(fmap), _lib.dptr(means),
                              _lib.dptr(ws), need, _lib.current_stream()))
        torch.cuda.synchronize()
        return fmap, means

    fmap, means = call(a, b)
    assert (fmap >= 0).all() and (fmap <= 1).all() and (means > 0).all()
    for k in range(n):
        one_map, one_mean = call(a[k:k + 1].contiguous(), b[k:k + 1].contiguous())
        assert torch.equal(one_map[0], fmap[k]) and torch.equal(one_mean[0], means[k])
    assert torch.equal(call(a, b, with_map=False)[1], means)
    again_map, again_means = call(a, b)
    assert torch.equal(again_map, fmap) and torch.equal(again_means, means)
    assert torch.allclose(means.double(), fmap.double().mean((1, 2)), rtol=1e-6, atol=0)
    assert torch.equal(call(b, a)[0], fmap)                            # symmetric in its two images
    assert abs(metrics.flip(a, b, pixels_per_degree=ppd) - float(means.double().mean())) == 0.0
    assert L.r2l_flip(None, None, 0, H, W, 0., 1., 0., 0., 1., 0., ppd, None, None, None, 0, None) == 0


def test_stacks_have_no_halo_and_runs_repeat(pkg, built_lib, golden):
    """three frames in one call = three calls, bit for bit; no map = the same means; twice = the same bits"""
    a0, b0, ppd, _ = _case(golden, 3)
    _stack_checks(a0, b0, ppd)


def test_stacks_at_the_largest_radius(pkg, built_lib, edges):
    """the same on three 33 x 129 frames at radii (16, 15), through a NaN-filled workspace of exactly the reported size"""
    k = EDGES.index((118.0, (16, 15), (33, 129)))
    a0, b0, ppd = _edge_case(edges, k)
    assert _radii(ppd) == (16, 15) and tuple(a0.shape[1:3]) == (33, 129)
    _stack_checks(a0, b0, ppd)


@pytest.mark.parametrize('k', range(len(EDGES)))
def test_edge_case(pkg, built_lib, edges, k):
    """map and mean of every natural pair of flip_edges.npz against the reference's float64 result, at the radii EDGES names"""
    from efficient_nerf_amd import metrics
    want_ppd, radii, shape = EDGES[k]
    a, b, ppd = _edge_case(edges, k)
    want = edges[f'map64_{k}']
    assert ppd == want_ppd and want.shape == shape and _radii(ppd) == radii
    mean, fmap = metrics.flip(a, b, pixels_per_degree=ppd, return_map=True)
    got = fmap[0].cpu().numpy().astype(np.float64)
    assert got.shape == want.shape
    band = max(float(edges[f'band_{j}']) for j in range(len(EDGES)) if EDGES[j][0] == want_ppd)
    err, err_mean = np.abs(got - want).max(), abs(mean - float(edges[f'mean64_{k}']))
    print(f'edge case {k} {shape} pixels_per_degree {ppd:.2f} radii {radii}: L_inf {err:.3e} = {err / band:.2f} band ({band:.2e}), mean off by '
          f'{err_mean:.3e} = {err_mean / band:.2f} band (mean {mean:.6f})')
    assert np.isfinite(got).all()
    assert err <= 4 * band and err_mean <= 4 * band


def test_a_nan_pixel_reaches_the_reference_s_box_and_an_inf_is_clamped(pkg, built_lib, golden, edges):
    """a[20, 30, 1] = NaN, b[5, 5, 0] = +Inf at radii (10, 9): NaN exactly where the reference's map is NaN, the other pixels within
    the band, a NaN mean, the same mean bits with and without a map"""
    from efficient_nerf_amd import _lib, metrics
    a, b, ppd = _edge_case(edges, NAN_CASE)
    want = edges[f'map64_{NAN_CASE}']
    nan = np.isnan(want)
    box = np.zeros(want.shape, dtype=bool)
    box[NAN_BOX] = True
    assert _radii(ppd) == (10, 9) and want.shape == (48, 56) and np.array_equal(nan, box) and np.isnan(float(edges[f'mean64_{NAN_CASE}']))
    assert torch.isnan(a).sum() == 1 and torch.isinf(b).sum() == 1
    mean, fmap = metrics.flip(a, b, pixels_per_degree=ppd, return_map=True)
    got_nan = torch.isnan(fmap[0]).cpu().numpy()
    got = fmap[0].cpu().numpy().astype(np.float64)
    rows, cols = np.flatnonzero(got_nan.any(1)), np.flatnonzero(got_nan.any(0))
    band = max([float(edges[f'band_{NAN_CASE}'])] + [float(golden[f'band_{j}']) for j in NATURAL if float(golden[f'ppd_{j}']) == ppd])
    err = np.abs(got - want)[~nan & ~got_nan].max()
    print(f'NaN case: {int(got_nan.sum())} NaN pixels in rows {rows.min()} .. {rows.max()}, columns {cols.min()} .. {cols.max()} (the reference: '
          f'{int(nan.sum())} in rows 10 .. 30, columns 20 .. 40); finite pixels L_inf {err:.3e} = {err / band:.2f} band ({band:.2e}); mean {mean}')
    assert np.array_equal(got_nan, nan)
    assert err <= 4 * band
    assert np.isnan(mean)
    assert np.array_equal(torch.isnan(metrics.flip(b, a, pixels_per_degree=ppd, return_map=True)[1][0]).cpu().numpy(), nan)
    L = _lib.lib()
    H, W = want.shape
    need = L.r2l_flip_workspace_floats(H, W, ppd)
    means = []
    for with_map in (True, False):
        ws = torch.full((need,), float('nan'), device='cuda')
        out = torch.full((1, H, W), -1., device='cuda') if with_map else None
        m = torch.full((1,), -1., device='cuda')
        _lib.check(L.r2l_flip(_lib.dptr(a), _lib.dptr(b), 1, H, W, 0., 1., 0., 0., 1., 0., ppd, _lib.dptr(out), _lib.dptr(m), _lib.dptr(ws), need,
                              _lib.current_stream()))
        torch.cuda.synchronize()
        means.append(m)
        if with_map:
            assert torch.equal(out.view(torch.int32), fmap.view(torch.int32))
    assert torch.isnan(means[0]).all() and torch.equal(means[0].view(torch.int32), means[1].view(torch.int32))


def test_identity_constants_equal_premapped_copies(pkg, built_lib, golden):
    """rescale=True on the rescaled case = rescale=False on copies mapped beforehand in the reference's operation order"""
    from efficient_nerf_amd import metrics
    a, b, ppd, resc = _case(golden, RESCALED)
    assert resc
    pre = lambda x: ((2 / (x.max() - x.min())) * (x - x.min())) + (-1)
    _, by_call = metrics.flip(a, b, pixels_per_degree=ppd, rescale=True, return_map=True)
    _, on_copies = metrics.flip(pre(a), pre(b), pixels_per_degree=ppd, rescale=False, return_map=True)
    gap = (by_call - on_copies).abs().max().item()
    print(f'rescale=True against pre-mapped copies: L_inf {gap:.3e}')
    assert gap <= 4 * _band(golden, RESCALED)
    _, as_is = metrics.flip(a, b, pixels_per_degree=ppd, return_map=True)
    assert (as_is - by_call).abs().max().item() > 1e-3                 # the rescale is not a no-op on this pair
    const = torch.full_like(a, 0.25)
    assert np.isnan(metrics.flip(const, b, pixels_per_degree=ppd, rescale=True))      # max = min: 2 / 0 * 0, as the reference's


# ---- the command line ----------------------------------------------------------------------------------------------------------
SIZE, N_TRAIN, N_TEST, ANGLE = 16, 16, 3, 0.6911
NET = ['--model_name', 'R2L', '--dataset_type', 'blender', '--white_bkgd', '--testskip', '1', '--netdepth', '8', '--netwidth', '64',
       '--n_sample_per_ray', '4', '--multires', '4', '--use_residual', '--trial.ON', '--trial.body_arch', 'resmlp']
TRAIN = ['--data_mode', 'rays', '--N_rand', '2', '--N_iters', '4', '--i_testset', '2', '--i_weights', '4', '--i_print', '1']
TEST_LINE = re.compile(r'^\[TEST\] Iter (\d+) TestPSNR (\S+) TestPSNRv2 (\S+) BestPSNRv2 (\S+) \(Iter (\d+)\) TestSSIM (\S+) TestFLIP (\d\.\d{4}) '
                       r'TrainHistPSNR (\S+) LR (\d\.\d{8}) Time (\S+)s$')


@pytest.fixture(scope='module')
def scene(pkg, built_lib, tmp_path_factory):
    """16 x 16 RGBA views of a soft-edged disc on cameras around the origin: 16 train views (one shard of 4096 rays) and three
    test views"""
    from efficient_nerf_amd import convert_data as CD
    from efficient_nerf_amd.frontend import pose_spherical, write_png
    root = tmp_path_factory.mktemp('flip_cli')
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
    assert len(paths) == 1
    return {'root': str(root), 'datadir': str(d), 'shards': f'{d}_real_train'}


def _train(scene, expname, extra=()):
    """train() in this process on seeded generators (the command line seeds nothing, as the reference's does not)"""
    from efficient_nerf_amd import train as T
    from efficient_nerf_amd.frontend import parse_args
    lines = []
    np.random.seed(5)
    torch.manual_seed(5)
    T.train(parse_args(NET + TRAIN + ['--datadir', scene['datadir'], '--datadir_kd', scene['shards'], '--basedir', scene['root'],
                                      '--expname', expname] + list(extra)), log=lines.append)
    ck = torch.load(os.path.join(scene['root'], expname, 'weights', 'ckpt.tar'), map_location='cpu', weights_only=False)
    return lines, ck


@pytest.fixture(scope='module')
def trained(scene):
    return _train(scene, 'with_flip', ['--test_flip'])


def test_training_reports_test_flip_and_ends_on_the_same_bits(scene, trained):
    lines, ck = trained
    tests = [TEST_LINE.match(ln) for ln in lines if ln.startswith('[TEST] Iter')]
    assert len(tests) == 2 and all(tests), [ln for ln in lines if ln.startswith('[TEST]')]
    assert [int(m.group(1)) for m in tests] == [2, 4] and all(0. < float(m.group(7)) <= 1. for m in tests)
    plain_lines, plain = _train(scene, 'without')
    assert not any('TestFLIP' in ln for ln in plain_lines) and sum(ln.startswith('[TEST] Iter') for ln in plain_lines) == 2
    assert ck['global_step'] == plain['global_step'] == 4
    for key in ('network_fn_state_dict',):
        assert list(ck[key]) == list(plain[key]) and all(torch.equal(ck[key][k], plain[key][k]) for k in ck[key])
    flat = lambda o: [o] if torch.is_tensor(o) else [t for v in (o.values() if isinstance(o, dict) else o if isinstance(o, (list, tuple)) else [])
                                                     for t in flat(v)]
    with_, without = flat(ck['optimizer_state_dict']), flat(plain['optimizer_state_dict'])
    assert len(with_) == len(without) > 0 and all(torch.equal(s, t) for s, t in zip(with_, without))
    # the fields in front of TestFLIP are those of the run without it
    strip = lambda ln: re.sub(r' Time \S+s$', '', re.sub(r'TestFLIP \S+ ', '', ln))
    assert [strip(ln) for ln in lines if ln.startswith('[TEST] Iter')] == [strip(ln) for ln in plain_lines if ln.startswith('[TEST] Iter')]


def test_render_only_prints_test_flip_of_the_rescaled_stacks(scene, trained):
    from efficient_nerf_amd import metrics, train as T
    from efficient_nerf_amd.frontend import parse_args
    ck = os.path.join(scene['root'], 'with_flip', 'weights', 'ckpt.tar')
    argv = NET + ['--datadir', scene['datadir'], '--render_only', '--render_test', '--precision', 'fp32', '--pretrained_ckpt', ck,
                  '--basedir', scene['root']]
    runs = {}
    for name, extra in (('flip', ['--test_flip']), ('plain', [])):
        r = subprocess.run(['timeout', '-k', '10', '240', sys.executable, os.path.join(ROOT, 'main.py')] + argv + ['--expname', name] + extra,
                           cwd=scene['root'], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        runs[name] = [ln for ln in r.stdout.splitlines() if ln.startswith('[TEST]')]
    assert len(runs['flip']) == len(runs['plain']) == 1
    got = re.search(r'^\[TEST\] TestPSNR (\S+) TestPSNRv2 (\S+) TestSSIM (\S+) TestFLIP (\S+)$', runs['flip'][0])
    assert got, runs['flip']
    assert re.search(r'TestSSIM (\S+)$', runs['plain'][0]) and runs['flip'][0].startswith(runs['plain'][0] + ' TestFLIP ')
    rgbs = torch.tensor(np.load(os.path.join(scene['root'], 'flip', 'gen_img', 'rgbs.npy'))).cuda()
    test, missing = T.load_test_split(parse_args(argv), device=rgbs.device)
    assert missing is None and rgbs.shape == test[2].shape == (N_TEST, SIZE, SIZE, 3)
    want = metrics.flip(rgbs, test[2], rescale=True)
    print(f'{runs["flip"][0]}; metrics.flip(rgbs.npy, ground truth, rescale=True) = {want:.6f}, as they are: {metrics.flip(rgbs, test[2]):.6f}')
    assert got.group(4) == f'{want:.4f}' and 0. < want <= 1.
