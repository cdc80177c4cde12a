"""GPU: a non-finite ray through the NeRF teacher's pipeline.  The reference decides: every output of every ray is NaN
exactly where float32 torch on the CPU has NaN (oracle.render_rays / teacher_render), and every other ray of the call keeps its bits.
The MLP kernels' ReLU (fmaxf, v_max in the generated chains) drops a NaN; nerf_mark_nonfinite_kernel behind every MLP launch writes NaN
into `raw` of a ray whose point or view-direction embedding holds one, and the scan kernels carry it on as torch does.

Every case takes its masks from the oracle and first asserts that they are the table's (tests/nonfinite_cases.py: poisons 0-3 and 5 make
every output of the ray NaN; poison 4, rays_d = 0, makes the view directions 0 / 0 and leaves the density branch finite: rgb_map, rgb0 and
disp_map NaN, acc_map = acc0 = depth_map = 0, z_std finite).  It then checks (1) the NaN masks of every key the oracle also returns,
element for element, and no new infinity, (2) that every unpoisoned ray is int32-equal, in every key, to the same call with each poisoned
ray replaced by a copy of its clean neighbour, (3) that the engine is in the same mode after both calls, and (4) that every slot of the
four sentinel-filled maps was written and none behind them.  Clean rays: rgb_map within 1e-4 of the oracle (tests/test_teacher_gpu.py).

70 rays x (12 + 10) samples: rays cross the chain kernels' 256-point tiles in both passes (12 samples: ray 21 and 42; 22: ray 11); the
poisons sit on ray 0, 11, 21, 22, 42 and 69.  The second shape, 5 rays x (64 + 128), takes the scan kernels' other instantiations."""
import functools

import pytest
import torch

import nonfinite_cases as NC
from oracle import r2l_oracle as O

pytestmark = pytest.mark.gpu

MODES = ('fp16x3', 'fp16x1', 'fp16_fp8', 'fp16x3_asm', 'fp16_mix')
N, S0, NI = 70, 12, 10
POSITIONS = (0, 11, 21, 22, 42, 69)
SHIFTS = (0, 3)
KEYS = ('rgb_map', 'disp_map', 'acc_map', 'depth_map', 'rgb0', 'disp0', 'acc0', 'z_std', 'z_samples', 'z_vals', 'raw')
MAPS = ('rgb_map', 'disp_map', 'acc_map', 'depth_map')
TOL_RGB = 1e-4


@functools.lru_cache(None)
def _states():
    return O.make_nerf_state(1, W=256), O.make_nerf_state(2, W=256)


@functools.lru_cache(None)
def _rays(shift):
    ro, rd, _ = NC.frame_rays(12, 12, N)
    return NC.poisoned_pair(ro, rd, POSITIONS, shift)


def _assert_table(ref, kinds, n):
    """the oracle's masks are the table's"""
    for r in range(n):
        for k in NC.TEACHER_KEYS:
            nan = torch.isnan(ref[k][r])
            want = False if r not in kinds else NC.TEACHER_NAN_D0[k] if kinds[r] == 4 else True
            assert bool(nan.all()) == want and bool(nan.any()) == want, (r, kinds.get(r), k, ref[k][r])
        if kinds.get(r) == 4:
            assert ref['acc_map'][r] == 0 and ref['acc0'][r] == 0 and ref['depth_map'][r] == 0


@functools.lru_cache(None)
def _oracle(shift):
    bo, bd, _, _, kinds = _rays(shift)
    with torch.no_grad():
        ref = O.render_rays(*_states(), bo, bd, N_samples=S0, N_importance=NI, white_bkgd=True)
    _assert_table(ref, kinds, N)
    return ref


def _engine(mode, s0=S0, ni=NI, skip=False, **kw):
    from efficient_nerf_amd import NeRFEngine, PRECISIONS
    eng = NeRFEngine(12, 12, O.focal_from_angle(12), N_samples=s0, N_importance=ni, precision=PRECISIONS[mode], **kw).load_state_dicts(*_states())
    if skip:
        eng.set_skip_rgb0(True)
    return eng


def _with_sentinels(eng, monkeypatch):
    """the engine's four maps go into sentinel-filled buffers with a guard band behind them: [(out, whole)] of the latest call"""
    made = []

    def outs(n):
        made[:] = [NC.sentinel_like(shape, eng.device) for shape in ((n, 3), (n,), (n,), (n,))]
        return tuple(o for o, _ in made)

    monkeypatch.setattr(eng, '_outs', outs)
    return made


def _check(eng, made, bad, dup, ref, kinds, what, keys=KEYS):
    n = bad[0].shape[0]
    got = {k: v.clone() for k, v in eng.render_rays(bad[0].cuda(), bad[1].cuda(), extras=True).items()}
    torch.cuda.synchronize()
    assert all(NC.written_exactly(o, w) for o, w in made), (what, 'slots unwritten, or written behind the end')                    # (4)
    mode = (eng.precision, eng.precision_coarse)
    twin = eng.render_rays(dup[0].cuda(), dup[1].cuda(), extras=True)
    clean = NC.clean_mask(n, kinds)
    err = float((got['rgb_map'].cpu() - ref['rgb_map'])[clean].abs().max())
    print(f'{what}: rgb_map NaN on rays {torch.isnan(got["rgb_map"]).any(-1).nonzero().flatten().tolist()}, clean rays L_inf vs the oracle {err:.3e}')
    for k in keys:
        if k not in got:
            assert k == 'rgb0' and eng._rgb0_skipped()
            continue
        g = got[k].cpu()
        assert torch.equal(torch.isnan(g), torch.isnan(ref[k])), (what, k, 'NaN mask', torch.isnan(g).reshape(n, -1).any(-1).nonzero().flatten().tolist())   # (1)
        assert NC.no_new_inf(g, ref[k]), (what, k, 'an infinity the oracle does not have')
        assert NC.int32_equal(got[k], twin[k], clean.cuda()), (what, k, 'an unpoisoned ray changed its bits')                        # (2)
    assert (eng.precision, eng.precision_coarse) == mode                                                                              # (3)
    assert err <= TOL_RGB, (what, err)


@pytest.mark.parametrize('skip', [False, True], ids=['rgb0', 'skip_rgb0'])
@pytest.mark.parametrize('mode', MODES)
def test_given_rays_in_every_mode(pkg, mode, skip, monkeypatch):
    """render_rays(extras=True) on the 70 rays, both rotations of the poisons, with and without the coarse view branch"""
    eng = _engine(mode, skip=skip)
    made = _with_sentinels(eng, monkeypatch)
    for shift in SHIFTS:
        bo, bd, do, dd, kinds = _rays(shift)
        _check(eng, made, (bo, bd), (do, dd), _oracle(shift), kinds, f'{mode} skip_rgb0 {skip} shift {shift}')
    eng.close()


@pytest.mark.parametrize('mode', MODES)
def test_five_rays_of_192_samples(pkg, mode, monkeypatch):
    """(64, 128) samples, 5 rays: ray 1 and ray 3 poisoned, three pairs of poisons"""
    eng = _engine(mode, 64, 128)
    made = _with_sentinels(eng, monkeypatch)
    ro, rd, _ = NC.frame_rays(12, 12, 5, theta=70.)
    for pair in ((0, 4), (1, 5), (2, 3)):
        bo, bd, do, dd = ro.clone(), rd.clone(), ro.clone(), rd.clone()
        kinds = dict(zip((1, 3), pair))
        for r, k in kinds.items():
            NC.poison_ray(bo, bd, r, k)
            do[r], dd[r] = ro[r + 1], rd[r + 1]
        with torch.no_grad():
            ref = O.render_rays(*_states(), bo, bd, N_samples=64, N_importance=128, white_bkgd=True)
        _assert_table(ref, kinds, 5)
        _check(eng, made, (bo, bd), (do, dd), ref, kinds, f'{mode} 5 x 192, poisons {pair}')
    eng.close()


@pytest.mark.parametrize('mode', MODES)
def test_render_with_a_poisoned_pose(pkg, mode, monkeypatch):
    """render(c2w) of the 12 x 12 frame with a NaN translation and with an infinity in one rotation entry: teacher_render's masks, every
    slot written; the same engine then renders the clean pose within the limit"""
    focal = O.focal_from_angle(12)
    eng = _engine(mode)
    made = _with_sentinels(eng, monkeypatch)
    good = torch.as_tensor(O.pose_spherical(30., -30., 4.))[:3, :4].float().contiguous()
    nan_t, inf_r = good.clone(), good.clone()
    nan_t[0, 3] = NC.NAN
    inf_r[1, 0] = NC.INF
    for name, c2w in (('nan_translation', nan_t), ('inf_rotation', inf_r)):
        ref = O.teacher_render(*_states(), 12, 12, focal, c2w, N_samples=S0, N_importance=NI, white_bkgd=True)
        assert all(torch.isnan(ref[k]).all() for k in NC.TEACHER_KEYS), name            # every ray of such a frame is poisoned
        got = eng.render(c2w, extras=True)
        torch.cuda.synchronize()
        assert all(NC.written_exactly(o, w) for o, w in made), (mode, name)
        for k in KEYS:
            assert torch.equal(torch.isnan(got[k].cpu()), torch.isnan(ref[k])) and NC.no_new_inf(got[k].cpu(), ref[k]), (mode, name, k)
    ref = O.teacher_render(*_states(), 12, 12, focal, good, N_samples=S0, N_importance=NI, white_bkgd=True)
    err = float((eng.render(good)['rgb_map'].cpu() - ref['rgb_map']).abs().max())
    assert err <= TOL_RGB, (mode, err)
    eng.close()


@pytest.mark.parametrize('mode', MODES)
def test_ndc_engine_with_a_ray_across_the_near_plane(pkg, mode, monkeypatch):
    """a forward-facing engine and one world ray with d_z = 0: nerf_ndc_rays_kernel divides by it.  The masks are those of teacher_render's
    ndc branch restated on given rays (view directions of the world rays, then oracle.ndc_rays, then render_rays on [0, 1])"""
    from efficient_nerf_amd import NeRFEngine, PRECISIONS
    H, W, focal = 10, 14, 18.0
    c2w = torch.eye(4)[:3, :4].clone()
    c2w[:, 3] = torch.tensor([0.1, -0.05, 0.3])
    ro, rd = O.get_rays(H, W, focal, c2w)
    ro, rd = ro.reshape(-1, 3).float()[:N].contiguous().clone(), rd.reshape(-1, 3).float()[:N].contiguous().clone()
    bo, bd, do, dd = ro.clone(), rd.clone(), ro.clone(), rd.clone()
    kinds = {22: 0}
    bd[22, 2] = 0.
    do[22], dd[22] = ro[23], rd[23]
    with torch.no_grad():
        vd = bd / torch.norm(bd, dim=-1, keepdim=True)
        o, d = O.ndc_rays(H, W, focal, 1., bo, bd)
        ref = O.render_rays(*_states(), o, d, near=0., far=1., viewdirs=vd, N_samples=S0, N_importance=NI, white_bkgd=True)
    assert torch.isfinite(vd).all()
    _assert_table(ref, kinds, N)             # every output of that ray is NaN, none of another
    eng = NeRFEngine(H, W, focal, near=0., far=1., ndc=True, N_samples=S0, N_importance=NI, precision=PRECISIONS[mode]).load_state_dicts(*_states())
    made = _with_sentinels(eng, monkeypatch)
    _check(eng, made, (bo, bd), (do, dd), ref, kinds, f'{mode} ndc')
    eng.close()


def test_choose_precision_ends_on_the_same_rung(pkg):
    """`auto` on the poisoned rays and on the set with duplicates ends on the same mode: its comparisons count a NaN on both sides as agreement"""
    bo, bd, do, dd, _ = _rays(0)
    names = []
    for ro, rd in ((bo, bd), (do, dd)):
        eng = _engine('fp16x3')
        names.append(eng.choose_precision(ro.cuda(), rd.cuda())[0])
        eng.close()
    print('auto on the poisoned set / with duplicates:', names)
    assert names[0] == names[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the watch: poisoned rays at the strided indices it samples
# ---------------------------------------------------------------------------------------------------------------------------------
WATCH_RAYS = 35                                   # of 70: every second ray (NeRFEngine._strided)
WATCH_POS = (0, 10, 22, 34, 42, 68)


@pytest.mark.parametrize('mode', ['fp16x1', 'fp16_fp8', 'fp16_mix', 'fp16x3_asm'])
def test_spot_check_with_poisoned_rays_among_the_sampled(pkg, mode, monkeypatch):
    """spot_check in every watched mode (the plain comparison with fp16x3, fp16_mix against three passes, fp16x3_asm stage by stage through
    _x3_pair): both renders give the same NaN masks, so the watch passes under the mode's limits with finite differences and the mode
    stays; with the NaN mask of the reference render's rgb_map altered -- a NaN ray finite, or a clean ray NaN -- it fails"""
    from efficient_nerf_amd import NeRFEngine, PRECISIONS
    ro, rd, _ = NC.frame_rays(12, 12, N)
    bo, bd, _, _, kinds = NC.poisoned_pair(ro, rd, WATCH_POS, 0)
    bo, bd = bo.cuda(), bd.cuda()
    eng = _engine(mode)
    idx = eng._strided(N, WATCH_RAYS, 'cuda')
    assert set(kinds) <= set(idx.tolist())
    got = eng.render_rays(bo, bd)
    assert int(torch.isnan(got['rgb_map'][idx]).all(-1).sum()) == 6 and int(torch.isnan(got['acc_map'][idx]).sum()) == 5
    before = (eng.precision, eng.precision_coarse)
    ok, d = eng.spot_check(bo, bd, got, n_rays=WATCH_RAYS)
    print(f'{mode}: watch ok {ok}, {d}')
    assert ok and all(d[k] == d[k] and d[k] < 1e-3 for k in eng.WATCH_KEYS) and (eng.precision, eng.precision_coarse) == before
    if mode in ('fp16x1', 'fp16_fp8'):             # by hand: the sampled rays in fp16x3, the elements that are numbers on both sides
        mine = {k: got[k][idx].clone() for k in eng.WATCH_KEYS}
        eng.set_precision(PRECISIONS['fp16x3'])
        ref = eng.render_rays(bo[idx].contiguous(), bd[idx].contiguous())
        for k in eng.WATCH_KEYS:
            m = ~torch.isnan(ref[k])
            assert torch.equal(torch.isnan(mine[k]), ~m) and d[k] == float((mine[k] - ref[k])[m].abs().max()), k
        eng.set_precision(PRECISIONS[mode])

    ref_mode = PRECISIONS['fp16x3_asm'] if mode == 'fp16_mix' else PRECISIONS['fp16x3']
    real = NeRFEngine.render_rays
    for row, value in ((0, 0.5), (1, NC.NAN)):      # sampled ray 0 is poisoned (ray 0), sampled ray 1 (ray 2) is clean
        def altered(self, *a, _row=row, _value=value, **kw):
            out = real(self, *a, **kw)
            if self.precision == ref_mode and self.precision_coarse == ref_mode:
                out['rgb_map'][_row, 2] = _value
            return out

        monkeypatch.setattr(NeRFEngine, 'render_rays', altered)
        ok, d = eng.spot_check(bo, bd, got, n_rays=WATCH_RAYS)
        monkeypatch.setattr(NeRFEngine, 'render_rays', real)
        assert not ok and d['rgb_map'] != d['rgb_map'], (mode, row, value, ok, d)
        assert (eng.precision, eng.precision_coarse) == before
    eng.close()
