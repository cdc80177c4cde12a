"""CPU: teacher training on LLFF scenes without a device -- the order in which RayBatches hands out the rows of the reference's ray
bank, the split and the bounds, the command line's refusals, the argument checks of nerf_train_batch_rays, and the recorded rows of
the reference's bank (tests/golden/llff_teacher/rows.npz, tools/make_llff_teacher_golden.py) against the fixture they were cut from."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FERN = ['--config', os.path.join(ROOT, 'configs', 'fern.txt')]
LEGO = ['--config', os.path.join(ROOT, 'configs', 'lego.txt')]
SCENE = os.path.join(ROOT, 'tests', 'golden', 'llff', 'scene')


def _stub_batches(TT, n_img, H, W, N_rand, lines):
    """a RayBatches whose three device hooks stay on the host: next() returns the window's bank rows"""

    class Stub(TT.RayBatches):
        def _upload(self, image_bytes, poses):
            self.uploaded = (tuple(image_bytes.shape), tuple(poses.shape))

        def _set_order(self):
            self._order = self.perm

        def _launch(self, begin, rows):
            return self._order[begin:begin + rows].clone()

    return Stub(torch.zeros((n_img, H, W, 3), dtype=torch.uint8), torch.zeros((n_img, 3, 5)), 37.5, N_rand, True, device='cpu', log=lines.append)


def _reference_stream(n, N_rand, steps, lines):
    """main.py:1152-1162, 1199-1210 on a bank whose row r holds r: [(the step's row numbers)]"""
    rays_rgb = np.broadcast_to(np.arange(n, dtype=np.float32)[:, None, None], (n, 3, 3)).copy()
    np.random.shuffle(rays_rgb)
    i_batch = 0
    rays_rgb = torch.Tensor(rays_rgb)
    out = []
    for _ in range(steps):
        batch = rays_rgb[i_batch:i_batch + N_rand]
        batch = torch.transpose(batch, 0, 1)
        assert bool((batch[0] == batch[2]).all())
        out.append(batch[2][:, 0].long())
        i_batch += N_rand
        if i_batch >= rays_rgb.shape[0]:
            lines.append('Shuffle data after an epoch!')
            rand_idx = torch.randperm(rays_rgb.shape[0])
            rays_rgb = rays_rgb[rand_idx]
            i_batch = 0
    return out


@pytest.mark.parametrize('N_rand,short', [(1024, 384), (960, 960)])
def test_ray_batches_follow_the_references_index_stream(pkg, N_rand, short):
    """two and a half epochs over the fixture's 9,600 training rays: the same rows in the same order as the reference's shuffled
    bank, its short last batch (384 rows at N_rand 1024), the wrap at i_batch >= n -- behind a full batch when N_rand divides n
    (960) -- the log line, and both random streams left where the reference leaves them"""
    from efficient_nerf_amd import train_teacher as TT
    n_img, H, W = 8, 30, 40
    n, steps = n_img * H * W, 25
    np.random.seed(5)
    torch.manual_seed(7)
    want_lines = []
    want = _reference_stream(n, N_rand, steps, want_lines)
    follow = (np.random.rand(), float(torch.rand(1)))
    np.random.seed(5)
    torch.manual_seed(7)
    lines = []
    rb = _stub_batches(TT, n_img, H, W, N_rand, lines)
    assert rb.n == n and rb.uploaded == ((n_img, H, W, 3), (n_img, 3, 4)) and rb.perm.dtype == torch.int64
    got = [rb.next() for _ in range(steps)]
    assert (np.random.rand(), float(torch.rand(1))) == follow
    assert [len(g) for g in got] == [len(w) for w in want]
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    assert [len(g) for g in got[:10]] == [N_rand] * 9 + [short] and len(got[10]) == N_rand         # the epoch's last batch, the next one
    assert lines == want_lines == ['Shuffle data after an epoch!'] * 2
    assert rb.i_batch == 5 * N_rand
    for e in range(2):                                         # an epoch hands out every row once
        assert torch.equal(torch.sort(torch.cat(got[10 * e:10 * e + 10]))[0], torch.arange(n))
    assert not torch.equal(torch.cat(got[:10]), torch.cat(got[10:20]))


def test_ray_batches_refuse_other_inputs(pkg):
    from efficient_nerf_amd import R2LError
    from efficient_nerf_amd import train_teacher as TT
    with pytest.raises(R2LError):
        TT.RayBatches(torch.zeros((2, 4, 4, 4), dtype=torch.uint8), torch.zeros((2, 3, 4)), 10., 8, True, device='cpu')
    with pytest.raises(R2LError):
        TT.RayBatches(torch.zeros((2, 4, 4, 3)), torch.zeros((2, 3, 4)), 10., 8, True, device='cpu')
    with pytest.raises(R2LError):
        TT.RayBatches(torch.zeros((2, 4, 4, 3), dtype=torch.uint8), torch.zeros((3, 3, 4)), 10., 8, True, device='cpu')


def test_split_and_bounds_of_the_fixture(pkg):
    """main.py:903-919 restated: every llffhold-th view held out, validation = test, near / far 0, 1 under NDC and 0.9 min(bds),
    max(bds) with --no_ndc; llffhold 0 keeps the loader's own view"""
    from efficient_nerf_amd import llff
    from efficient_nerf_amd.train_teacher import llff_split_and_bounds
    scene = llff.load_scene(SCENE, 8)
    images, bds = scene.images, scene.bds
    for llffhold in (8, 3):
        i_test = np.arange(images.shape[0])[::llffhold]
        i_val = i_test
        i_train = np.array([i for i in np.arange(int(images.shape[0])) if (i not in i_test and i not in i_val)])
        for no_ndc in (False, True):
            if no_ndc:
                near = np.ndarray.min(bds) * .9
                far = np.ndarray.max(bds) * 1.
            else:
                near = 0.
                far = 1.
            got = llff_split_and_bounds(scene, llffhold, no_ndc)
            assert np.array_equal(got[0], i_train) and np.array_equal(got[1], i_val) and np.array_equal(got[2], i_test)
            assert got[3] == float(near) and got[4] == float(far) and isinstance(got[3], float)
    got = llff_split_and_bounds(scene, 8, True)
    assert len(got[0]) == 8 and list(got[2]) == [0, 8] and 0 < got[3] < got[4]
    got = llff_split_and_bounds(scene, 0, False)
    assert list(got[2]) == [scene.i_test] and len(got[0]) == len(images) - 1 and scene.i_test not in got[0]


def test_fern_config_holds_the_references_values(pkg):
    from efficient_nerf_amd import frontend as fe
    a = fe.parse_args(FERN)
    assert (a.dataset_type, a.factor, a.llffhold, a.N_rand, a.N_samples, a.N_importance, a.use_viewdirs, a.raw_noise_std, a.no_batching,
            a.no_ndc, a.white_bkgd, a.expname, a.datadir) == \
        ('llff', 8, 8, 1024, 64, 64, True, 1., False, False, False, 'fern_test', './data/nerf_llff_data/fern')


def test_check_supported_lets_llff_with_use_batching_through(pkg):
    from efficient_nerf_amd import frontend as fe
    from efficient_nerf_amd import train_teacher as TT
    quiet = ['--i_video', '1000000']
    assert TT.check_supported(fe.parse_args(FERN + quiet)) is None
    assert TT.check_supported(fe.parse_args(FERN + quiet + ['--no_ndc'])) is None
    for argv, line in ((LEGO + quiet + ['--dataset_type', 'llff'], '--dataset_type llff: teacher training is built for Blender scenes'),
                       (FERN + quiet + ['--dataset_type', 'blender'], 'use_batching'),
                       (FERN + quiet + ['--select_pixel_mode', 'rand_patch'], '--select_pixel_mode rand_patch'),
                       (FERN + ['--i_video', '50', '--N_iters', '100'], '--i_video 50 falls inside this run'),
                       (FERN + quiet + ['--model_name', 'R2L'], '--model_name R2L')):
        with pytest.raises(SystemExit) as e:
            TT.check_supported(fe.parse_args(argv))
        assert line in str(e.value) and '\n' not in str(e.value)
    with pytest.raises(SystemExit) as e:                       # LLFF with no_batching says how LLFF does train
        TT.check_supported(fe.parse_args(LEGO + quiet + ['--dataset_type', 'llff']))
    assert 'use_batching' in str(e.value)


def test_a_scene_the_loader_refuses_ends_in_its_line(pkg, tmp_path):
    """--spherify and a missing scene fail as the loader makes them fail, before any device is asked for"""
    from efficient_nerf_amd import frontend as fe
    from efficient_nerf_amd import train_teacher as TT
    quiet = ['--i_video', '1000000', '--basedir', str(tmp_path)]
    with pytest.raises(SystemExit) as e:
        TT.train(fe.parse_args(FERN + quiet + ['--datadir', SCENE, '--spherify']), log=lambda *a: None)
    assert '--spherify' in str(e.value) and 'not built' in str(e.value)
    with pytest.raises(SystemExit) as e:
        TT.train(fe.parse_args(FERN + quiet + ['--datadir', str(tmp_path / 'nowhere')]), log=lambda *a: None)
    assert 'poses_bounds.npy' in str(e.value)
    with pytest.raises(SystemExit) as e:
        TT.train(fe.parse_args(FERN + quiet + ['--datadir', SCENE, '--factor', '4']), log=lambda *a: None)
    assert 'images_4' in str(e.value)


def test_batch_rays_checks_its_arguments(pkg, built_lib):
    """R2L_EINVAL with the entry point's name in the message on NULL, misaligned or out-of-range arguments, before any device is
    looked for"""
    from efficient_nerf_amd import _lib
    L = _lib.lib()
    err = lambda: L.r2l_last_error().decode()
    p, q = C.c_void_p(0x1000), C.c_void_p(0x100000)
    f = L.nerf_train_batch_rays
    good = [p, 8, 30, 40, p, 37.5, p, 1024, 1, 1., q, q, q, q, None]

    def call(**kw):
        names = ['images', 'n_img', 'H', 'W', 'poses', 'focal', 'order', 'rows', 'ndc', 'near', 'rays_o', 'rays_d', 'viewdirs', 'target', 'stream']
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return f(*args)

    for kw in (dict(images=None), dict(poses=None), dict(order=None), dict(rays_o=None), dict(rays_d=None), dict(target=None),
               dict(n_img=0), dict(H=0), dict(W=-1), dict(rows=-1), dict(focal=0.), dict(focal=-3.), dict(focal=float('nan')),
               dict(poses=C.c_void_p(0x1002)), dict(order=C.c_void_p(0x1004)), dict(rays_o=C.c_void_p(0x100001)),
               dict(rays_d=C.c_void_p(0x100002)), dict(viewdirs=C.c_void_p(0x100003)), dict(target=C.c_void_p(0x100001)),
               dict(rows=1 << 40)):
        assert call(**kw) == -1, kw
        assert 'nerf_train_batch_rays' in err(), (kw, err())
    assert call(focal=0.) == -1 and 'focal' in err()
    assert call(order=C.c_void_p(0x1004)) == -1 and 'aligned' in err()
    assert call(rows=-1) == -1 and 'rows=-1' in err()


def test_golden_rows_are_the_fixtures_pixels(pkg, golden_dir):
    """the recorded rows of the reference's bank: the colours are the fixture's bytes / 255 at image-major, row, column positions
    over the training views, the origins the poses' last columns, and the view directions and NDC rows agree with a float64
    restatement of main.py:154 and helpers:260-279 on the recorded world rays"""
    from efficient_nerf_amd import llff
    from efficient_nerf_amd.train_teacher import llff_split_and_bounds
    g = np.load(os.path.join(golden_dir, 'llff_teacher', 'rows.npz'))
    scene = llff.load_scene(SCENE, 8)
    i_train = llff_split_and_bounds(scene, 8, False)[0]
    H, W, focal = scene.hwf
    assert (int(g['H']), int(g['W']), float(g['focal']), int(g['n'])) == (H, W, focal, len(i_train) * H * W)
    rows = g['rows']
    assert rows.shape == (256,) and rows[0] == 0 and rows[-1] == len(i_train) * H * W - 1 and len(set(rows.tolist())) == 256
    img, pix = rows // (H * W), rows % (H * W)
    flat = scene.bytes[i_train].reshape(len(i_train), H * W, 3)
    assert np.array_equal(g['target'], (flat[img, pix] / 255.).astype(np.float32))
    assert np.array_equal(g['rays_o'], scene.poses[i_train][img, :3, 3])
    d, o = g['rays_d'].astype(np.float64), g['rays_o'].astype(np.float64)
    assert np.abs(g['viewdirs'] - d / np.linalg.norm(d, axis=-1, keepdims=True)).max() < 5e-7
    t = -(1. + o[:, 2]) / d[:, 2]
    o = o + t[:, None] * d
    o2 = np.stack([-1. / (W / (2. * focal)) * o[:, 0] / o[:, 2], -1. / (H / (2. * focal)) * o[:, 1] / o[:, 2], 1. + 2. / o[:, 2]], -1)
    d2 = np.stack([-1. / (W / (2. * focal)) * (d[:, 0] / d[:, 2] - o[:, 0] / o[:, 2]),
                   -1. / (H / (2. * focal)) * (d[:, 1] / d[:, 2] - o[:, 1] / o[:, 2]), -2. / o[:, 2]], -1)
    assert np.abs(g['ndc_o'] - o2).max() < 2e-6 and np.abs(g['ndc_d'] - d2).max() < 2e-6
