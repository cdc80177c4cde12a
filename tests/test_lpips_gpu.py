"""GPU: LPIPS (v0.1, AlexNet trunk) on the library's kernels (csrc/r2l_lpips.hip, efficient-nerf_amd/metrics.py LPIPS) and TestLPIPS
on the [TEST] lines behind --test_lpips.

The yardstick is the oracle below: the formula as plain torch on the CPU (scaling layer, torchvision's AlexNet features with zero
padding and floor-mode pooling, channel normalisation with eps 1e-10 behind the square root, lin-weighted squared difference, mean
over the pixels, sum over the five layers), evaluated once in float64 and once in float32 on seeded weights (conv randn *
sqrt(2 / fan_in), biases uniform in +-0.1, lin uniform in [0, 1)) and seeded frames (a uniform in [-1, 1], b = clamp(a + 0.3 randn),
one pair of each stack with b = a).  The kernels and the float32 oracle are both float32 with different summation orders, so the
kernels' d and every d_k may sit 8 x the float32 oracle's own worst relative error (over the three sizes' non-identical pairs, d and
every d_k) from the float64 result; that single sample is close to rounding noise, hence the factor.  So that the rule cannot hide a
failure the float32 oracle must itself lie within 1e-5 relative of float64 on every one of them.  Agreement with the lpips package
on its released weights is not checked here: neither is available offline.

The pairs go through the workspace in groups whose size follows from the deepest feature map (plan() below restates the library's
arithmetic): 8 at SIZES, and 7, 2 and 1 at GROUP_SIZES, the smallest near-square, non-square frames with those groups (800 x 800 and
1008 x 756 have 2, LLFF's 504 x 378 has 7, everything from 1039 x 1039 up has 1).  Those are held to the same rule, with the limit
from their own float32 oracle; stacks longer than a group and no multiple of it must give every pair the bits it has alone, in
either order of the two stacks, through a NaN-filled workspace of exactly the reported size.  A NaN pixel makes its own pair's d and
every d_k NaN, as it does the oracle's (F.relu passes a NaN on; so must the layer kernel's ReLU), and leaves the other pairs of its
group their bits."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((31, 31), (37, 50), (131, 97))          # the minimum (7, 3, 1, 1, 1); non-square, edge pixels dropped; row tiles and two-level sums
GROUP_SIZES = {(411, 415): (7, 9), (747, 751): (2, 5), (1039, 1043): (1, 3)}      # pairs per group, and a stack longer than one and no multiple of it
FEATURE_MAPS = {(31, 31): ((7, 7), (3, 3), (1, 1)), (37, 50): ((8, 11), (3, 5), (1, 2)), (131, 97): ((32, 23), (15, 11), (7, 5)),
                (411, 415): ((102, 103), (50, 51), (24, 25)), (747, 751): ((186, 187), (92, 93), (45, 46)),
                (1039, 1043): ((259, 260), (129, 129), (64, 64))}
R2L_EINVAL = -1
N, IDENTICAL = 3, 1
CONVS = ((64, 3, 11, 4, 2), (192, 64, 5, 1, 2), (384, 192, 3, 1, 1), (256, 384, 3, 1, 1), (256, 256, 3, 1, 1))      # out, in, k, stride, pad
SHIFT, SCALE = (-.030, -.088, -.188), (.458, .448, .450)


def seeded_weights(seed=0):
    """5 conv weights, 5 biases, 5 lin vectors: the order r2l_lpips_create takes"""
    g = torch.Generator().manual_seed(seed)
    w = [torch.randn(o, i, k, k, generator=g) * (2 / (i * k * k)) ** .5 for o, i, k, _, _ in CONVS]
    b = [torch.rand(o, generator=g) * .2 - .1 for o, *_ in CONVS]
    lin = [torch.rand(o, generator=g) for o, *_ in CONVS]
    return w + b + lin


def frames(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(N, H, W, 3, generator=g) * 2 - 1
    b = (a + .3 * torch.randn(N, H, W, 3, generator=g)).clamp(-1, 1)
    b[IDENTICAL] = a[IDENTICAL]
    return a, b


def oracle(weights, a, b, dtype):
    """the six steps of the formula on the CPU in `dtype`: (d [N], d_k [N, 5]) in float64"""
    w, bias, lin = ([t.to(dtype) for t in weights[5 * j:5 * j + 5]] for j in range(3))
    shift, scale = (torch.tensor(v, dtype=dtype).view(1, 3, 1, 1) for v in (SHIFT, SCALE))

    def features(x):
        x = (x.permute(0, 3, 1, 2).to(dtype) - shift) / scale
        out = []
        for k, (_, _, _, stride, pad) in enumerate(CONVS):
            if k in (1, 2):
                x = F.max_pool2d(x, 3, 2)
            x = F.relu(F.conv2d(x, w[k], bias[k], stride=stride, padding=pad))
            out.append(x)
        return out

    fa, fb = features(a), features(b)
    layers = []
    for k in range(5):
        na, nb = (f / (torch.sqrt(torch.sum(f ** 2, dim=1, keepdim=True)) + 1e-10) for f in (fa[k], fb[k]))
        layers.append((lin[k].view(1, -1, 1, 1) * (na - nb) ** 2).sum(1).mean((1, 2)))
    layers = torch.stack(layers, 1)
    return layers.sum(1).double(), layers.double()


def plan(H, W):
    """csrc/r2l_lpips.hip's lpips_plan restated: (pairs per group, workspace floats).  Per image of a group the five feature maps,
    the two pooled maps and the largest patch matrix; per pair conv 1's partial sums and 8 floats of d_k"""
    conv = lambda v, k: (v + 2 * CONVS[k][4] - CONVS[k][2]) // CONVS[k][3] + 1
    pool = lambda v: (v - 3) // 2 + 1
    h, w, ins, outs = H, W, [], []
    for k in range(5):
        if k in (1, 2):
            h, w = pool(h), pool(w)
        ins.append(h * w)
        h, w = conv(h, k), conv(w, k)
        outs.append(h * w)
    group = min(8, max(1, -(-4096 // outs[4])))
    per_image = sum(outs[k] * CONVS[k][0] for k in range(5)) + ins[1] * CONVS[0][0] + ins[2] * CONVS[1][0] + \
        max(outs[k] * CONVS[k][1] * CONVS[k][2] ** 2 for k in range(5))
    return group, 2 * group * per_image + group * (-(-outs[0] // 32)) + group * 8


def rel(got, want):
    """the worst relative error of d and of every d_k over the non-identical pairs; entries whose exact value is 0 must be 0"""
    worst = 0.
    for g, w in zip(got, want):
        g, w = (torch.as_tensor(v, dtype=torch.float64).cpu() for v in (g, w))
        keep = [k for k in range(N) if k != IDENTICAL]
        g, w = g[keep].reshape(-1), w[keep].reshape(-1)
        assert torch.all(g[w == 0] == 0)
        worst = max(worst, float(((g - w).abs() / w)[w != 0].max()))
    return worst


@pytest.fixture(scope='module')
def weights():
    return seeded_weights()


@pytest.fixture(scope='module')
def cases(weights):
    """per size the frames and both oracles; 'limit': 8 x the float32 oracle's worst relative error over all of them"""
    out, worst = {}, 0.
    for j, (H, W) in enumerate(SIZES):
        a, b = frames(H, W, seed=10 + j)
        want, own = oracle(weights, a, b, torch.float64), oracle(weights, a, b, torch.float32)
        err = rel(own, want)
        assert err <= 1e-5, f'{H} x {W}: the float32 oracle is {err:.2e} from float64: pick other seeds'
        assert all(0.05 < float(want[0][k]) < 1. for k in range(N) if k != IDENTICAL) and float(want[0][IDENTICAL]) == 0.
        out[(H, W)] = dict(a=a, b=b, want=want, oracle_err=err)
        worst = max(worst, err)
    out['oracle_err'], out['limit'] = worst, 8 * worst
    return out


@pytest.fixture(scope='module')
def group_cases(weights):
    """the same per size of GROUP_SIZES, with a limit of their own"""
    out, worst = {}, 0.
    for j, (H, W) in enumerate(GROUP_SIZES):
        a, b = frames(H, W, seed=20 + j)
        want, own = oracle(weights, a, b, torch.float64), oracle(weights, a, b, torch.float32)
        err = rel(own, want)
        assert err <= 1e-5, f'{H} x {W}: the float32 oracle is {err:.2e} from float64: pick other seeds'
        assert all(0.05 < float(want[0][k]) < 1. for k in range(N) if k != IDENTICAL) and float(want[0][IDENTICAL]) == 0.
        out[(H, W)] = dict(a=a, b=b, want=want, oracle_err=err)
        worst = max(worst, err)
    out['oracle_err'], out['limit'] = worst, 8 * worst
    return out


@pytest.fixture(scope='module')
def metric(pkg, built_lib, weights):
    from efficient_nerf_amd import metrics
    m = metrics.LPIPS(weights)
    yield m
    m.close()


def run(metric, a, b, **kw):
    """(mean, d [N], d_k [N, 5]) of one call"""
    mean, layers = metric(a.cuda(), b.cuda(), return_layers=True, **kw)
    return mean, metric.last_d.clone(), layers


@pytest.mark.parametrize('size', SIZES)
def test_parity_with_the_float64_oracle(pkg, built_lib, metric, cases, size):
    """d and every d_k of the three pairs against float64; the identical pair is exactly 0; the feature maps have the sizes the
    formula gives"""
    from efficient_nerf_amd import _lib
    c = cases[size]
    H, W = size
    sizes = FEATURE_MAPS[size]
    need = _lib.lib().r2l_lpips_workspace_floats(H, W)
    p1, p2, p3 = (h * w for h, w in sizes)
    assert need >= 2 * p1 * (363 + 64) + 2 * p2 * 192 + 2 * p3 * (384 + 256 + 256)
    mean, d, layers = run(metric, c['a'], c['b'])
    err = rel((d, layers), c['want'])
    print(f'{H} x {W} (feature maps {sizes}): float32 oracle {c["oracle_err"]:.3e} (worst of the sizes {cases["oracle_err"]:.3e}), HIP {err:.3e}, '
          f'limit {cases["limit"]:.3e}; d = {[round(float(v), 6) for v in d]}')
    assert torch.isfinite(d).all() and torch.isfinite(layers).all()
    assert float(d[IDENTICAL]) == 0. and torch.all(layers[IDENTICAL] == 0.)
    assert err <= cases['limit']
    assert mean == float(d.double().mean())


def test_symmetric_repeatable_and_independent_of_the_stack(pkg, built_lib, metric, cases):
    """d(a, b) = d(b, a), two calls, a pair alone and the call without the layers: all the same bits"""
    for size in SIZES[1:]:
        a, b = cases[size]['a'].cuda(), cases[size]['b'].cuda()
        mean, d, layers = run(metric, a, b)
        mean_ba, d_ba, layers_ba = run(metric, b, a)
        assert torch.equal(d, d_ba) and torch.equal(layers, layers_ba) and mean == mean_ba
        _, d_again, layers_again = run(metric, a, b)
        assert torch.equal(d, d_again) and torch.equal(layers, layers_again)
        for k in range(N):
            _, d_one, layers_one = run(metric, a[k:k + 1], b[k:k + 1])
            assert torch.equal(d_one[0], d[k]) and torch.equal(layers_one[0], layers[k])
        assert metric(a, b) == mean and torch.equal(metric.last_d, d)
        assert np.isnan(metric(a[:0], b[:0]))                  # n_img = 0: no launch, no value
    # small frames go through the workspace up to 8 pairs at a time: 10 pairs are two groups, each pair as it is alone
    a, b = cases[SIZES[0]]['a'].cuda(), cases[SIZES[0]]['b'].cuda()
    _, d, layers = run(metric, a, b)
    pick = [k % N for k in range(10)]
    mean_10, layers_10 = metric(a[pick].contiguous(), b[pick].contiguous(), return_layers=True)
    assert torch.equal(metric.last_d, d[pick]) and torch.equal(layers_10, layers[pick]) and mean_10 == float(d[pick].double().mean())


@pytest.mark.parametrize('size', list(GROUP_SIZES))
def test_parity_at_groups_of_7_2_and_1(pkg, built_lib, metric, group_cases, size):
    """the same rule where the workspace holds 7, 2 and 1 pairs at a time; the reported workspace is the plan's, so the group is"""
    from efficient_nerf_amd import _lib
    c = group_cases[size]
    H, W = size
    sizes = FEATURE_MAPS[size]
    group, floats = plan(H, W)
    need = _lib.lib().r2l_lpips_workspace_floats(H, W)
    p1, p2, p3 = (h * w for h, w in sizes)
    assert group == GROUP_SIZES[size][0] and min(8, -(-4096 // p3)) == group
    assert need >= group * (2 * p1 * (363 + 64) + 2 * p2 * 192 + 2 * p3 * (384 + 256 + 256)) and need == floats
    mean, d, layers = run(metric, c['a'], c['b'])
    err = rel((d, layers), c['want'])
    print(f'{H} x {W} (feature maps {sizes}, {group} pairs a group): float32 oracle {c["oracle_err"]:.3e} (worst of the sizes '
          f'{group_cases["oracle_err"]:.3e}), HIP {err:.3e}, limit {group_cases["limit"]:.3e}, HIP / limit {err / group_cases["limit"]:.3f}; '
          f'd = {[round(float(v), 6) for v in d]}')
    assert torch.isfinite(d).all() and torch.isfinite(layers).all()
    assert float(d[IDENTICAL]) == 0. and torch.all(layers[IDENTICAL] == 0.)
    assert err <= group_cases['limit']
    assert mean == float(d.double().mean())


def bits(t):
    return t.contiguous().view(torch.int32)


def raw_call(metric, a, b, floats):
    """one r2l_lpips call through a NaN-filled workspace of `floats` floats: (return code, d, layers), d and layers pre-filled with -1"""
    from efficient_nerf_amd import _lib
    n, H, W = a.shape[:3]
    ws = torch.full((floats,), float('nan'), device='cuda')
    d, layers = torch.full((n,), -1., device='cuda'), torch.full((n, 5), -1., device='cuda')
    rc = _lib.lib().r2l_lpips(metric._ctx, _lib.dptr(a), _lib.dptr(b), n, H, W, 0., 1., 0., 0., 1., 0., _lib.dptr(d), _lib.dptr(layers), _lib.dptr(ws),
                              floats, _lib.current_stream())
    torch.cuda.synchronize()
    return rc, d, layers


@pytest.mark.parametrize('size', list(GROUP_SIZES))
def test_a_pair_does_not_depend_on_its_group_below_8(pkg, built_lib, metric, group_cases, size):
    """a stack of more than one group and no multiple of it: every pair has the bits it has alone, d(a, b) = d(b, a); a NaN-filled
    workspace of exactly the reported size gives the same bits, one float less is refused before any launch"""
    from efficient_nerf_amd import _lib
    group, n_stack = GROUP_SIZES[size]
    assert n_stack > group and (n_stack % group or group == 1) and plan(*size)[0] == group
    a, b = group_cases[size]['a'].cuda(), group_cases[size]['b'].cuda()
    alone = [run(metric, a[k:k + 1], b[k:k + 1]) for k in range(N)]
    d = torch.cat([one[1] for one in alone])
    layers = torch.cat([one[2] for one in alone])
    pick = [k % N for k in range(n_stack)]
    sa, sb = a[pick].contiguous(), b[pick].contiguous()
    mean, d_stack, layers_stack = run(metric, sa, sb)
    assert torch.equal(d_stack, d[pick]) and torch.equal(layers_stack, layers[pick]) and mean == float(d[pick].double().mean())
    _, d_ba, layers_ba = run(metric, sb, sa)
    assert torch.equal(d_ba, d_stack) and torch.equal(layers_ba, layers_stack)
    need = _lib.lib().r2l_lpips_workspace_floats(*size)
    rc, d_raw, layers_raw = raw_call(metric, sa, sb, need)
    assert rc == 0 and torch.equal(bits(d_raw), bits(d_stack)) and torch.equal(bits(layers_raw), bits(layers_stack))
    rc, d_raw, layers_raw = raw_call(metric, sa, sb, need - 1)
    assert rc == R2L_EINVAL and 'workspace' in _lib.lib().r2l_last_error().decode()
    assert torch.all(d_raw == -1.) and torch.all(layers_raw == -1.)          # nothing was launched


def _nan_checks(metric, weights, a, b, pick, at):
    """stacks a[pick], b[pick] with a NaN at a_stack[at]: that pair's d and d_k are NaN as the float64 oracle's are, every other pair
    keeps the bits it has without the NaN"""
    sa, sb = a[pick].contiguous().cuda(), b[pick].contiguous().cuda()
    _, d, layers = run(metric, sa, sb)
    assert torch.isfinite(d).all() and torch.isfinite(layers).all()
    sa[at] = float('nan')
    k = at[0]
    want_d, want_layers = oracle(weights, sa[k:k + 1].cpu(), sb[k:k + 1].cpu(), torch.float64)
    assert torch.isnan(want_d).all() and torch.isnan(want_layers).all()
    mean, d_nan, layers_nan = run(metric, sa, sb)
    others = [j for j in range(len(pick)) if j != k]
    print(f'{tuple(sa.shape)} with a NaN at {at}: d = {[float(v) for v in d_nan]}, d_k of that pair = {[float(v) for v in layers_nan[k]]}')
    assert torch.isnan(d_nan[k]) and torch.isnan(layers_nan[k]).all() and np.isnan(mean)
    assert torch.equal(bits(d_nan[others]), bits(d[others])) and torch.equal(bits(layers_nan[others]), bits(layers[others]))
    _, d_ba, layers_ba = run(metric, sb, sa)
    assert torch.isnan(d_ba[k]) and torch.isnan(layers_ba[k]).all() and torch.equal(bits(d_ba[others]), bits(d[others]))


def test_a_nan_pixel_makes_its_pair_nan_and_no_other(pkg, built_lib, metric, weights, cases, group_cases):
    """37 x 50, a[0, 5, 7, 1] = NaN; 411 x 415, the NaN in the last pair of 9 (a group of 7 and one of 2)"""
    size = SIZES[1]
    _nan_checks(metric, weights, cases[size]['a'], cases[size]['b'], list(range(N)), (0, 5, 7, 1))
    size = (411, 415)
    n_stack = GROUP_SIZES[size][1]
    _nan_checks(metric, weights, group_cases[size]['a'], group_cases[size]['b'], [k % N for k in range(n_stack)], (n_stack - 1, 200, 300, 1))
    _nan_checks(metric, weights, group_cases[size]['a'], group_cases[size]['b'], [k % N for k in range(n_stack)], (3, 0, 0, 2))


def test_a_dead_layer_gives_zero_not_nan(pkg, built_lib, weights, cases):
    """layer 3's bias at -1e3: all its features are 0, d_3 = 0.0 exactly, everything finite, the other layers still match"""
    from efficient_nerf_amd import metrics
    dead = list(weights)
    dead[5 + 2] = torch.full_like(weights[5 + 2], -1e3)
    size = SIZES[1]
    a, b = cases[size]['a'], cases[size]['b']
    want = oracle(dead, a, b, torch.float64)
    assert torch.all(want[1][:, 2] == 0) and torch.all(want[1][0, :2] > 0)
    m = metrics.LPIPS(dead)
    _, d, layers = run(m, a, b)
    m.close()
    assert torch.isfinite(d).all() and torch.isfinite(layers).all() and torch.all(layers[:, 2] == 0.)
    err = rel((d, layers), want)
    print(f'dead layer 3 at {size}: HIP {err:.3e}, limit {cases["limit"]:.3e}; d_k of pair 0 = {[float(v) for v in layers[0]]}')
    assert err <= cases['limit']


def test_rescale_is_the_reference_s_mapping(pkg, built_lib, metric, weights, cases):
    """rescale=True = the oracle on stacks rescaled in float32 as main.py:361-363 does"""
    size = SIZES[1]
    a, b = cases[size]['a'] * .4 + .5, cases[size]['b'] * .35 + .45          # frames in about [0, 1], as the renders are
    pre = lambda x: ((2 / (x.max() - x.min())) * (x - x.min())) + (-1)
    want = oracle(weights, pre(a), pre(b), torch.float64)
    _, d, layers = run(metric, a, b, rescale=True)
    err = rel((d, layers), want)            # the pair with b = a is nearly identical after the mapping: its tiny d is all cancellation
    _, d_plain, _ = run(metric, a, b)
    print(f'rescale=True at {size}: HIP {err:.3e}, limit {cases["limit"]:.3e}; d = {[float(v) for v in d]}, as they are {[float(v) for v in d_plain]}')
    assert err <= cases['limit']
    assert float((d - d_plain).abs().max()) > 1e-3          # the mapping is not a no-op on these stacks


# ---- the command line ----------------------------------------------------------------------------------------------------------
SIZE, N_TRAIN, N_TEST, ANGLE = 32, 4, 3, 0.6911
NET = ['--model_name', 'R2L', '--dataset_type', 'blender', '--white_bkgd', '--testskip', '1', '--netdepth', '8', '--netwidth', '64',
       '--n_sample_per_ray', '4', '--multires', '4', '--use_residual', '--trial.ON', '--trial.body_arch', 'resmlp']
TRAIN = ['--data_mode', 'rays', '--N_rand', '1', '--N_iters', '4', '--i_testset', '2', '--i_weights', '4', '--i_print', '1']
TEST_LINE = re.compile(r'^\[TEST\] Iter (\d+) TestPSNR (\S+) TestPSNRv2 (\S+) BestPSNRv2 (\S+) \(Iter (\d+)\) TestSSIM (\S+) TestLPIPS (\d\.\d{4}) '
                       r'TrainHistPSNR (\S+) LR (\d\.\d{8}) Time (\S+)s$')


@pytest.fixture(scope='module')
def scene(pkg, built_lib, weights, tmp_path_factory):
    """32 x 32 RGBA views of a soft-edged disc on cameras around the origin: four train views (one shard of 4096 rays), three test
    views, and the seeded weights as one LPIPS state_dict"""
    from efficient_nerf_amd import convert_data as CD
    from efficient_nerf_amd.frontend import pose_spherical, write_png
    root = tmp_path_factory.mktemp('lpips_cli')
    d = root / 'scene'
    y, x = np.meshgrid(np.arange(SIZE), np.arange(SIZE), indexing='ij')
    for split, n in (('train', N_TRAIN), ('test', N_TEST)):
        (d / split).mkdir(parents=True)
        frames_ = []
        for k in range(n):
            theta = 360. * k / n + (0. if split == 'train' else 17.)
            img = np.zeros((SIZE, SIZE, 4), dtype=np.uint8)
            for c in range(3):
                img[..., c] = np.clip(127.5 + 127.5 * np.sin(0.2 * x + 0.15 * y * (c + 1) + np.radians(theta) + c), 0, 255)
            img[..., 3] = np.clip(255. * (15.5 - np.hypot(x - 15.5, y - 15.5)) / 6., 0, 255)
            write_png(str(d / split / f'r_{k}.png'), img)
            frames_.append({'file_path': f'./{split}/r_{k}', 'transform_matrix': pose_spherical(theta, -30., 4.).tolist()})
        with open(d / f'transforms_{split}.json', 'w') as fp:
            json.dump({'camera_angle_x': ANGLE, 'frames': frames_}, fp)
    paths = CD.convert(CD.parse_args(['--splits', 'train', '--datadir', str(d), '--full_res', '--seed', '1']), log=lambda *a: None)
    assert len(paths) == 1
    names = ('slice1.0', 'slice2.3', 'slice3.6', 'slice4.8', 'slice5.10')
    sd = {f'net.{s}.weight': weights[k] for k, s in enumerate(names)}
    sd.update({f'net.{s}.bias': weights[5 + k] for k, s in enumerate(names)})
    sd.update({f'lin{k}.model.1.weight': weights[10 + k].view(1, -1, 1, 1) for k in range(5)})
    torch.save(sd, str(root / 'lpips_alex.pth'))
    return {'root': str(root), 'datadir': str(d), 'shards': f'{d}_real_train', 'weights': str(root / 'lpips_alex.pth')}


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
    return _train(scene, 'with_lpips', ['--test_lpips', '--lpips_weights', scene['weights']])


def test_training_reports_test_lpips_and_ends_on_the_same_bits(scene, trained):
    lines, ck = trained
    tests = [TEST_LINE.match(ln) for ln in lines if ln.startswith('[TEST] Iter')]
    assert len(tests) == 2 and all(tests), [ln for ln in lines if ln.startswith('[TEST]')]
    assert [int(m.group(1)) for m in tests] == [2, 4] and all(0. < float(m.group(7)) < 10. for m in tests)
    plain_lines, plain = _train(scene, 'without')
    assert not any('TestLPIPS' in ln for ln in plain_lines) and sum(ln.startswith('[TEST] Iter') for ln in plain_lines) == 2
    assert ck['global_step'] == plain['global_step'] == 4
    for key in ('network_fn_state_dict',):
        assert list(ck[key]) == list(plain[key]) and all(torch.equal(ck[key][k], plain[key][k]) for k in ck[key])
    flat = lambda o: [o] if torch.is_tensor(o) else [t for v in (o.values() if isinstance(o, dict) else o if isinstance(o, (list, tuple)) else [])
                                                     for t in flat(v)]
    with_, without = flat(ck['optimizer_state_dict']), flat(plain['optimizer_state_dict'])
    assert len(with_) == len(without) > 0 and all(torch.equal(s, t) for s, t in zip(with_, without))
    # the fields around TestLPIPS are those of the run without it
    strip = lambda ln: re.sub(r' Time \S+s$', '', re.sub(r'TestLPIPS \S+ ', '', ln))
    assert [strip(ln) for ln in lines if ln.startswith('[TEST] Iter')] == [strip(ln) for ln in plain_lines if ln.startswith('[TEST] Iter')]


def test_render_only_prints_test_lpips_between_ssim_and_flip(scene, trained, weights):
    from efficient_nerf_amd import metrics, train as T
    from efficient_nerf_amd.frontend import parse_args
    ck = os.path.join(scene['root'], 'with_lpips', 'weights', 'ckpt.tar')
    argv = NET + ['--datadir', scene['datadir'], '--render_only', '--render_test', '--precision', 'fp32', '--pretrained_ckpt', ck,
                  '--basedir', scene['root']]
    lp = ['--test_lpips', '--lpips_weights', scene['weights']]
    runs = {}
    for name, extra in (('lpips', lp), ('both', lp + ['--test_flip']), ('plain', [])):
        r = subprocess.run(['timeout', '-k', '10', '240', sys.executable, os.path.join(ROOT, 'main.py')] + argv + ['--expname', name] + extra,
                           cwd=scene['root'], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        runs[name] = [ln for ln in r.stdout.splitlines() if ln.startswith('[TEST]')]
    assert len(runs['lpips']) == len(runs['both']) == len(runs['plain']) == 1
    assert re.search(r'^\[TEST\] TestPSNR (\S+) TestPSNRv2 (\S+) TestSSIM (\S+)$', runs['plain'][0]), runs['plain']      # the parent's format
    got = re.search(r'^\[TEST\] TestPSNR (\S+) TestPSNRv2 (\S+) TestSSIM (\S+) TestLPIPS (\S+)$', runs['lpips'][0])
    assert got and runs['lpips'][0].startswith(runs['plain'][0] + ' TestLPIPS '), runs['lpips']
    both = re.search(r'^\[TEST\] TestPSNR (\S+) TestPSNRv2 (\S+) TestSSIM (\S+) TestLPIPS (\S+) TestFLIP (\S+)$', runs['both'][0])
    assert both and both.group(4) == got.group(4) and runs['both'][0].startswith(runs['lpips'][0] + ' TestFLIP '), runs['both']
    rgbs = torch.tensor(np.load(os.path.join(scene['root'], 'lpips', 'gen_img', 'rgbs.npy'))).cuda()
    test, missing = T.load_test_split(parse_args(argv), device=rgbs.device)
    assert missing is None and rgbs.shape == test[2].shape == (N_TEST, SIZE, SIZE, 3)
    m = metrics.LPIPS(metrics.load_lpips_weights(scene['weights']))
    want = m(rgbs, test[2], rescale=True)
    print(f'{runs["both"][0]}; metrics.LPIPS(rgbs.npy, ground truth, rescale=True) = {want:.6f}, as they are: {m(rgbs, test[2]):.6f}')
    m.close()
    assert got.group(4) == f'{want:.4f}' and want > 0.
