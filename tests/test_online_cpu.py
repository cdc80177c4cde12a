"""CPU: the parts of online distillation that need no device -- the argument checks of r2l_rand_rays, the command lines --kd_online
refuses, the pixel draw (Philox4x32-10 + mulhi, restated here in numpy and held against the generator's published known answers),
OnlineTeacherSource's host draws and its watch on a stub engine."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R2L_EINVAL = -1


# ---- the numpy mirror of the kernel's draw (tests/test_online_gpu.py imports it) -----------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter = four words, key =
    two words, each a uint32 scalar or array; returns the four output words as uint64 arrays holding 32-bit values"""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    mask, s32 = np.uint64(0xffffffff), np.uint64(32)
    c = [np.asarray(x, dtype=np.uint64) for x in counter]
    k0, k1 = (np.asarray(x, dtype=np.uint64) for x in key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                    # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & mask, (p0 >> s32) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + W0) & mask, (k1 + W1) & mask
    return c


def lo_hi(v):
    v = int(v) & (2 ** 64 - 1)
    return np.uint64(v & 0xffffffff), np.uint64(v >> 32)


def rand_pixels(seed, step, n, n_pix):
    """pixel index of rays 0 .. n - 1: mulhi32(word 0 of Philox4x32-10 with counter (k_lo, k_hi, step_lo, step_hi) and key (seed_lo,
    seed_hi), n_pix)"""
    k = np.arange(n, dtype=np.uint64)
    x = philox4x32_10([k & np.uint64(0xffffffff), k >> np.uint64(32), *lo_hi(step)], lo_hi(seed))[0]
    return ((x * np.uint64(n_pix)) >> np.uint64(32)).astype(np.int64)


def host_rays(poses, focals, H, W, seed, step, n):
    """what r2l_rand_rays computes, in numpy float32 with its operations in its order; returns (rays_o, rays_d, pixel)"""
    f32 = np.float32
    po, fo = np.asarray(poses, dtype=f32), np.asarray(focals, dtype=f32)
    pix = rand_pixels(seed, step, n, H * W)
    p = np.arange(n) % len(po)
    j, i = pix // W, pix % W
    dx = (i.astype(f32) - f32(W * .5)) / fo[p]
    dy = -((j.astype(f32) - f32(H * .5)) / fo[p])
    c = po[p]
    rd = np.stack([(dx * c[:, r, 0] + dy * c[:, r, 1]) + f32(-1.) * c[:, r, 2] for r in range(3)], -1)
    return c[:, :, 3].copy(), rd.astype(f32), pix


def test_philox_known_answers():
    """the known-answer vectors of Random123's kat_vectors for philox4x32 with 10 rounds: all zeros, all ones, and the digits of pi"""
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(x) for x in philox4x32_10(ctr, key)) == want
    # as arrays, one lane per vector
    got = philox4x32_10([np.array([k[0][w] for k in kat]) for w in range(4)], [np.array([k[1][w] for k in kat]) for w in range(2)])
    assert [tuple(int(got[w][v]) for w in range(4)) for v in range(3)] == [k[2] for k in kat]


def test_rand_pixels_mulhi():
    n_pix = 35
    pix = rand_pixels(7, 3, 1000, n_pix)
    x = philox4x32_10([np.arange(1000), np.zeros(1000), np.full(1000, 3), np.zeros(1000)], (7, 0))[0]
    assert pix.tolist() == [(int(v) * n_pix) >> 32 for v in x]
    assert pix.min() >= 0 and pix.max() < n_pix and len(set(pix.tolist())) == n_pix
    assert not np.array_equal(pix, rand_pixels(7, 4, 1000, n_pix)) and not np.array_equal(pix, rand_pixels(8, 3, 1000, n_pix))
    # a seed and a step beyond 32 bits reach the key's and the counter's high words
    assert not np.array_equal(rand_pixels(7 + (1 << 32), 3, 64, n_pix), pix[:64])
    assert not np.array_equal(rand_pixels(7, 3 + (1 << 32), 64, n_pix), pix[:64])


def test_rand_rays_checks_its_arguments(pkg, built_lib):
    """R2L_EINVAL with a message for each bad argument, before any device is looked for (this machine may have none)"""
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    err = lambda: L.r2l_last_error().decode()
    p, q, r = C.c_void_p(0x1000), C.c_void_p(0x100000), C.c_void_p(0x200000)
    good = dict(poses=p, focal=p, n_pose=3, H=5, W=7, seed=0, step=1, n=10, ro=q, rd=r, pix=None)
    call = lambda **kw: (lambda a: L.r2l_rand_rays(a['poses'], a['focal'], a['n_pose'], a['H'], a['W'], a['seed'], a['step'], a['n'], a['ro'],
                                                   a['rd'], a['pix'], None))(dict(good, **kw))
    for bad in (dict(poses=None), dict(focal=None), dict(ro=None), dict(rd=None), dict(n_pose=0), dict(n_pose=-2), dict(H=0), dict(W=0),
                dict(H=-1, W=-1), dict(H=1 << 16, W=1 << 15), dict(H=1 << 20, W=1 << 20), dict(n=-1)):
        assert call(**bad) == R2L_EINVAL, bad
        assert 'r2l_rand_rays' in err(), bad
    assert call(pix=C.c_void_p(0x1004)) == R2L_EINVAL and 'aligned' in err()
    # the largest grid the pixel draw covers passes the argument check: what answers an empty launch of it is the device check
    rc = call(H=(1 << 16) - 1, W=1 << 15, n=0, ro=None, rd=None)
    assert rc == 0 or 'r2l_rand_rays' not in err()


def _args(extra):
    return ['--model_name', 'R2L', '--config', os.path.join(ROOT, 'configs', 'lego_noview.txt'), '--kd_online'] + list(extra)


def test_flags_and_defaults(pkg):
    from efficient_nerf_amd import frontend as fe
    d = fe.parse_args([])
    assert (d.kd_online, d.teacher_ckpt, d.teacher_config, d.kd_online_poses, d.kd_online_seed, d.kd_online_watch, d.kd_online_split,
            d.no_rand_focal) == (False, '', '', 100, 0, 100, 4096, False)
    a = fe.parse_args(_args(['--teacher_ckpt', 'T.tar', '--kd_online_poses', '7', '--kd_online_seed', '5', '--kd_online_watch', '0',
                             '--kd_online_split', '256', '--no_rand_focal', '--teacher_config', 'X.txt']))
    assert (a.kd_online, a.teacher_ckpt, a.teacher_config, a.kd_online_poses, a.kd_online_seed, a.kd_online_watch, a.kd_online_split,
            a.no_rand_focal) == (True, 'T.tar', 'X.txt', 7, 5, 0, 256, True)


def test_the_three_refusals(pkg):
    """each a SystemExit of one line, from the command line's entry and from train() alike, before a device is touched"""
    from efficient_nerf_amd import frontend as fe, train as T
    cases = [(['--teacher_ckpt', 'T.tar', '--datadir_kd', 'DIR'], '--datadir_kd DIR'),
             ([], 'needs --teacher_ckpt'),
             (['--teacher_ckpt', 'T.tar', '--dataset_type', 'llff'], "--dataset_type llff: the random poses are Blender's hemisphere")]
    for extra, what in cases:
        for run in (lambda argv: fe.main(argv), lambda argv: T.train(fe.parse_args(argv), log=lambda *a: None)):
            with pytest.raises(SystemExit) as e:
                run(_args(extra))
            msg = str(e.value)
            assert what in msg and msg.startswith('--kd_online') and '\n' not in msg, msg


def test_teacher_flags_come_from_the_teacher_config(pkg, tmp_path):
    from efficient_nerf_amd import frontend as fe
    from efficient_nerf_amd.online import teacher_args
    a = fe.parse_args(_args(['--teacher_ckpt', 'T.tar', '--H', '32', '--precision', 'fp16x3', '--datadir', str(tmp_path)]))
    t = teacher_args(a)                                  # default: lego.txt beside the student's --config
    assert not a.use_viewdirs and t.use_viewdirs and (t.N_samples, t.N_importance, t.white_bkgd, t.half_res) == (64, 128, True, True)
    assert (t.H, t.precision, t.datadir) == (32, 'fp16x3', str(tmp_path)) and not fe.teacher_needs_generic(t)
    cfg = tmp_path / 'teacher.txt'
    cfg.write_text('use_viewdirs = True\nN_samples = 8\nN_importance = 16\nwhite_bkgd = True\n')
    a.teacher_config = str(cfg)
    t = teacher_args(a)
    assert (t.N_samples, t.N_importance, t.half_res) == (8, 16, False)
    a.teacher_config = str(tmp_path / 'missing.txt')
    with pytest.raises(SystemExit) as e:
        teacher_args(a)
    assert 'missing.txt' in str(e.value) and '\n' not in str(e.value)


# ---- OnlineTeacherSource on the host -----------------------------------------------------------------------------------------------
class StubEngine:
    """CPU tensors; render_rays is a fixed function of the rays and of the mode; spot_check fails `misses` times"""
    LADDER = ('fast', 'slow', 'exact')
    WATCH_RAYS = 4

    def __init__(self, misses=1):
        self.device = 'cpu'
        self.mode, self.misses = 0, misses
        self.calls = []

    @property
    def precision_name(self):
        return self.LADDER[self.mode]

    def set_skip_rgb0(self, on=True):
        self.calls.append(('skip_rgb0', on))

    def render_rays(self, ro, rd):
        self.calls.append(('render', self.mode))
        return {'rgb_map': torch.sigmoid(ro * 0.25 + rd) + float(self.mode)}

    def spot_check(self, ro, rd, got):
        self.calls.append(('check', self.mode))
        assert torch.equal(got['rgb_map'], torch.sigmoid(ro * 0.25 + rd) + float(self.mode))       # what was just rendered for these rays
        if self.misses > 0:
            self.misses -= 1
            return False, {'rgb_map': 0.5}
        return True, {'rgb_map': 0.}

    def step_down(self):
        self.calls.append(('step_down', self.mode))
        self.mode += 1
        return self.precision_name


def _source(eng, log, H=5, W=7, focal=6., n_pose=3, seed=2, **kw):
    from efficient_nerf_amd.online import OnlineTeacherSource
    rays = lambda poses, focals, step, n: tuple(torch.from_numpy(a) for a in host_rays(poses.numpy(), focals.numpy(), H, W, seed, step, n)[:2])
    return OnlineTeacherSource(eng, H, W, focal, n_pose=n_pose, seed=seed, log=log, rays_fn=rays, **kw)


def test_draws_are_rand_streams_formulae(pkg):
    """step t's poses and focals: per pose theta, phi, then the focal scale, from RandomState((seed, t)) with no loader poses skipped"""
    from efficient_nerf_amd.create_data import RandStream
    from efficient_nerf_amd.frontend import pose_spherical
    seed, f = 2, 6.
    src = _source(StubEngine(0), None, n_pose=4, seed=seed, focal=f)
    for t in (1, 2, 1000):
        poses, focals = src.draws(t)
        assert poses.shape == (4, 3, 4) and poses.dtype == torch.float32 and focals.shape == (4,) and focals.dtype == np.float64
        rs = np.random.RandomState((seed, t))
        stream = RandStream(seed=(seed, t), n_loader_poses=0)
        for p in range(4):
            theta, phi, scale = -180 + rs.rand() * 360, -90 + rs.rand() * 90, rs.rand() + 1
            assert -180 <= theta < 180 and -90 <= phi < 0 and 1 <= scale < 2
            assert torch.equal(poses[p], pose_spherical(theta, phi, 4)[:3, :4]) and torch.equal(poses[p], stream.rand_pose()[:3, :4])
            assert focals[p] == f * scale == f * stream.rand_focal_scale() and f <= focals[p] < 2 * f
    assert not torch.equal(src.draws(1)[0], src.draws(2)[0])
    assert not torch.equal(src.draws(1)[0], _source(StubEngine(0), None, n_pose=4, seed=seed + 1).draws(1)[0])
    # --no_rand_focal: the focal is f for every pose and the poses consume theta, phi only
    fixed = _source(StubEngine(0), None, n_pose=4, seed=seed, focal=f, use_rand_focal=False)
    poses, focals = fixed.draws(5)
    rs = np.random.RandomState((seed, 5))
    want = [pose_spherical(-180 + rs.rand() * 360, -90 + rs.rand() * 90, 4)[:3, :4] for _ in range(4)]
    assert focals.tolist() == [f] * 4 and all(torch.equal(a, b) for a, b in zip(poses, want))


def test_batch_is_a_function_of_seed_and_step(pkg):
    eng = StubEngine(0)
    src = _source(eng, None, watch_every=0)
    assert eng.calls == [('skip_rgb0', True)]
    a = src.batch(4, 50)
    poses, focals = src.draws(4)
    ro, rd, _ = host_rays(poses.numpy(), focals.astype(np.float32), 5, 7, 2, 4, 50)
    assert all(t.shape == (50, 3) and t.dtype == torch.float32 for t in a)
    assert np.array_equal(a[0].numpy(), ro) and np.array_equal(a[1].numpy(), rd) and torch.equal(a[2], torch.sigmoid(a[0] * 0.25 + a[1]))
    b = src.batch(5, 50)
    assert not torch.equal(a[1], b[1])
    fresh = _source(StubEngine(0), None, watch_every=0)
    assert all(torch.equal(x, y) for x, y in zip(b, fresh.batch(5, 50)))
    assert all(torch.equal(x, y) for x, y in zip(a, src.batch(4, 50)))       # step t again after t + 1 was asked for
    assert not any(c[0] == 'check' for c in eng.calls)   # watch_every = 0: never


def test_watch_miss_steps_down_once_and_renders_again(pkg):
    lines = []
    eng = StubEngine(misses=1)
    src = _source(eng, lines.append, watch_every=10)
    for step in (8, 9):
        src.batch(step, 20)
    assert [c[0] for c in eng.calls[1:]] == ['render', 'render'] and not lines       # not a watched step
    del eng.calls[:]
    ro, rd, target = src.batch(10, 20)
    assert eng.calls == [('render', 0), ('check', 0), ('step_down', 0), ('render', 1), ('check', 1)]
    assert torch.equal(target, torch.sigmoid(ro * 0.25 + rd) + 1.)              # the second render's
    assert len(lines) == 1 and '\n' not in lines[0]
    assert all(s in lines[0] for s in ('step 10', 'fast', 'slow', "'rgb_map': 0.5")), lines[0]
    assert src.checks == 2 and [(f['step'], f['from'], f['to']) for f in src.fallbacks] == [(10, 'fast', 'slow')]
    del eng.calls[:]
    src.batch(20, 20)                                     # the next watched step passes in the mode taken
    assert eng.calls == [('render', 1), ('check', 1)] and len(lines) == 1
