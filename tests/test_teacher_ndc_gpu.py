"""GPU: forward-facing teacher renders (`--dataset_type llff`, NeRFEngine(..., ndc=True); main.py:148-162) in EVERY precision mode.
They are the only renders that hand the layer-chain kernels GIVEN view directions -- those of the world rays, at points of the projected
rays -- which switches nerf_tile_load / nerf_tile_embed to p.viewdirs, forces the three-tile build of the fp16x1 chain and rules out the
one-statement nerf_chain_emb_kernel (csrc/nerf_capi.hip run_mlp).  Per point (run_network(..., viewdirs=)) and through the pipeline
against the CPU oracle, the second exit and the coarse stream without its view branch bit for bit, and `auto` / the watch on an NDC
engine (NeRFEngine._x3_pair has to re-evaluate the fine pass on the projected rays).

A wrong direction shows: with the neighbouring ray's directions the oracle's rgb_map moves by 8.4e-3 and the colour columns of raw by
0.036 on this frame; every comparison below asserts that sensitivity on its own reference before it asserts the tolerance.

Tolerances are those of the world-space tests of the same teacher family (tests/test_teacher_gpu.py): 2e-4 on raw (2e-5 for the
three-pass chain), 1e-4 on the composited maps, 2e-4 on z_vals, 5e-6 on rgb for the two fp32-grade modes."""
import functools
import math

import pytest
import torch

from oracle import r2l_oracle as O

pytestmark = pytest.mark.gpu

H, W, FOCAL = 10, 14, 18.0
NEAR, FAR = 0., 1.
MODES = ('fp16x3', 'fp16x3_asm', 'fp16_fp8', 'fp16x1', 'fp16_mix')
# (rays, N_samples, N_importance): 140 rays x 192 samples is a whole number of 128-point tiles, so the tail lanes need other counts;
# S = 67 puts a ray boundary inside every tile
SHAPES = {'n1': (1, 64, 128), 'n139': (139, 64, 128), 's67': (140, 17, 50), 'frame': (140, 64, 128)}
RAGGED = ('n1', 'n139', 's67')
RAW_TOL = {'fp16x3': 2e-4, 'fp16x3_asm': 2e-5, 'fp16_fp8': 2e-4, 'fp16x1': 2e-4, 'fp16_mix': 2e-4}
MAP_TOL = {'rgb_map': 1e-4, 'acc_map': 1e-4, 'rgb0': 1e-4, 'acc0': 1e-4, 'depth_map': 1e-4 * max(1., FAR), 'z_vals': 2e-4}
FP32_GRADE = 5e-6            # fp16x3 and fp16x3_asm on rgb (tests/test_teacher_gpu.py test_teacher_fp16x3_asm_mode)
SENSITIVITY = 20             # a wrong direction must move the reference by at least this many tolerances


def _c2w():
    c = torch.eye(4)[:3, :4].clone()
    c[:, 3] = torch.tensor([0.1, -0.05, 0.3])
    return c


@functools.lru_cache(None)
def _plain():
    return O.make_teacher_state(1), O.make_teacher_state(2)


@functools.lru_cache(None)
def _sparse():
    """a teacher most of whose fine tiles see no positive density on this frame (for the bitwise tests only: its rgb is too insensitive to
    the directions for a comparison with the oracle to mean much)"""
    sds = []
    for seed in (3, 4):
        sd = O.make_teacher_state(seed, sigma_bias_shift=0.)
        sd['alpha_linear.weight'] = sd['alpha_linear.weight'] * 64
        sd['alpha_linear.bias'] = sd['alpha_linear.bias'] * 64 + 0.5
        sds.append(sd)
    return tuple(sds)


@pytest.fixture(scope='module')
def frame(pkg):
    """world rays of the frame (CPU), the library's own projection of them (bit-exact against the reference: test_ndc_rays_bit_exact)
    copied to the CPU for the oracle, and the world rays' directions: both sides see the same points and directions"""
    from efficient_nerf_amd import ndc_rays
    ro, rd = O.get_rays(H, W, FOCAL, _c2w())
    ro, rd = ro.reshape(-1, 3).float().contiguous(), rd.reshape(-1, 3).float().contiguous()
    o, d = ndc_rays(H, W, FOCAL, 1., ro.cuda(), rd.cuda())
    vd = rd / rd.norm(dim=-1, keepdim=True)
    # the neighbouring ray's direction for every ray (of the whole frame, so that a single ray has a neighbour too)
    return dict(ro=ro, rd=rd, o=o.cpu(), d=d.cpu(), vd=vd, vd_wrong=torch.roll(vd, 1, 0))


_CACHE = {}


def _oracle(frame, shape, white=True, wrong=False):
    """O.render_rays on the first n projected rays of the frame with the (right or the neighbour's) directions; computed once"""
    key = ('render', shape, white, wrong)
    if key not in _CACHE:
        n, S0, NI = SHAPES[shape]
        t0, t1 = _plain()
        with torch.no_grad():
            _CACHE[key] = O.render_rays(t0, t1, frame['o'][:n], frame['d'][:n], near=NEAR, far=FAR, viewdirs=frame['vd_wrong' if wrong else 'vd'][:n],
                                        white_bkgd=white, N_samples=S0, N_importance=NI)
    return _CACHE[key]


def _raw64(frame, shape, which, z, zname):
    """the network in float64 on the float32 points o' + d' z, with the right and with the neighbour's directions; computed once"""
    key = ('raw', shape, which, zname)
    if key not in _CACHE:
        n = SHAPES[shape][0]
        o, d = frame['o'][:n], frame['d'][:n]
        pts = o[:, None, :] + d[:, None, :] * z.expand(n, z.shape[-1])[:, :, None]
        with torch.no_grad():
            _CACHE[key] = tuple(O.run_network(_plain()[which], pts, frame[k][:n], dtype=torch.float64) for k in ('vd', 'vd_wrong'))
    return _CACHE[key]


def _engine(shape, mode='fp16x3', white=True, ndc=True, sds=None, near=NEAR, far=FAR):
    from efficient_nerf_amd import NeRFEngine, PRECISIONS
    _, S0, NI = SHAPES[shape]
    eng = NeRFEngine(H, W, FOCAL, near=near, far=far, N_samples=S0, N_importance=NI, white_bkgd=white, ndc=ndc)
    eng.load_state_dicts(*(sds or _plain()))
    eng.set_precision(PRECISIONS[mode])
    return eng


def _bits(t):
    return t.contiguous().view(torch.int32)      # disp of an empty ray is 0 / 0 = NaN in the reference too (main.py:609-610)


def _fmt(d):
    return {k: f'{float(v):.2e}' for k, v in d.items()}


# ---- a. per point -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', RAGGED)
@pytest.mark.parametrize('mode', MODES)
def test_run_network_with_given_directions_vs_float64(pkg, frame, mode, shape):
    """run_network(which, o', d', z, viewdirs=vd) of both networks, with the shared coarse depths (stride 0) and with per-ray depths (the
    oracle's merged z_vals), against the network in float64 on the same float32 points: 2e-4 on raw, 2e-5 for the three-pass chain"""
    n = SHAPES[shape][0]
    eng = _engine(shape, mode)
    tol = RAW_TOL[mode]
    o, d, vd = (frame[k][:n].cuda() for k in ('o', 'd', 'vd'))
    errs = {}
    for zname, z in (('shared', eng.z_coarse), ('per ray', _oracle(frame, shape)['z_vals'])):
        assert z.shape == ((SHAPES[shape][1],) if zname == 'shared' else (n, SHAPES[shape][1] + SHAPES[shape][2]))
        for which in (0, 1):
            want, wrong = _raw64(frame, shape, which, z, zname)
            got = eng.run_network(which, o, d, z.cuda(), viewdirs=vd).cpu()
            assert got.shape == want.shape and bool(torch.isfinite(got).all())
            sens = (wrong - want)[..., :3].abs().max().item()
            errs[f'net {which}, {zname} z'] = err = (got - want).abs().max().item()
            assert sens >= SENSITIVITY * tol, (which, zname, sens)            # the comparison can fail: the neighbour's directions would
            assert err <= tol, (mode, shape, which, zname, err, f'(the neighbour\'s directions: {sens:.2e})')
    print(f'{mode} {shape}: raw L_inf from float64 {_fmt(errs)} (limit {tol:.0e}; the neighbour\'s directions move the colours by {sens:.2e})')
    eng.close()


def test_run_network_without_directions_is_nerf_run_network_bit_for_bit(pkg, frame):
    """viewdirs=None goes through nerf_run_network_dirs(..., NULL, ...): on a world-space engine bit for bit what nerf_run_network gives,
    in every mode, both networks, shared and per-ray depths, a ragged ray count"""
    from efficient_nerf_amd import PRECISIONS
    from efficient_nerf_amd._lib import check, current_stream, dptr, lib
    n = 139
    eng = _engine('n139', ndc=False, near=2., far=6.)
    ro, rd = frame['ro'][:n].cuda(), frame['rd'][:n].cuda()
    zr = eng.render_rays(ro, rd, extras=True)['z_vals'].clone()
    for mode in MODES:
        eng.set_precision(PRECISIONS[mode])
        for which in (0, 1):
            for z, stride in ((eng.z_coarse.cuda(), 0), (zr, zr.shape[1])):
                got = eng.run_network(which, ro, rd, z)
                S = z.shape[-1]
                want = torch.full((n, S, 4), float('nan'), device='cuda')
                check(lib().nerf_run_network(eng._ctx, which, dptr(ro), dptr(rd), dptr(z), stride, S, n, dptr(want), current_stream()))
                assert torch.equal(_bits(got), _bits(want)) and bool(torch.isfinite(got).all()), (mode, which, stride)
    eng.close()


# ---- b. pipeline --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,shape,white', [(m, s, True) for m in MODES for s in RAGGED] + [('fp16x1', 'n139', False)])
def test_ndc_pipeline_vs_oracle(pkg, frame, mode, shape, white):
    """render_rays(ro, rd, extras=True) and render(c2w) on an ndc=True engine against O.render_rays on the projected rays with the world
    rays' directions: every map, the coarse maps and the merged depths; the first n rays of render(c2w) are render_rays' bit for bit"""
    from efficient_nerf_amd import PRECISIONS
    n = SHAPES[shape][0]
    eng = _engine(shape, mode, white=white)
    ro, rd = frame['ro'][:n].cuda(), frame['rd'][:n].cuda()
    out = {k: v.clone() for k, v in eng.render_rays(ro, rd, extras=True).items()}
    ref, wrong = _oracle(frame, shape, white), _oracle(frame, shape, white, wrong=True)
    sens = (wrong['rgb_map'] - ref['rgb_map']).abs().max().item()
    errs = {k: (out[k].cpu() - ref[k]).abs().max().item() for k in MAP_TOL}
    print(f'{mode} {shape} white_bkgd={white}: L_inf from the oracle {_fmt(errs)}; the neighbour\'s directions move rgb_map by {sens:.2e}')
    assert sens >= SENSITIVITY * MAP_TOL['rgb_map'], sens
    for k, tol in MAP_TOL.items():
        assert out[k].shape == ref[k].shape and errs[k] <= tol, (k, errs[k])
    if mode in ('fp16x3', 'fp16x3_asm'):          # fp32-grade, and the two against each other
        assert errs['rgb_map'] <= FP32_GRADE, errs['rgb_map']
        eng.set_precision(PRECISIONS['fp16x3_asm' if mode == 'fp16x3' else 'fp16x3'])
        pair = (eng.render_rays(ro, rd)['rgb_map'] - out['rgb_map']).abs().max().item()
        eng.set_precision(PRECISIONS[mode])
        print(f'   fp16x3 against fp16x3_asm on rgb_map: {pair:.2e}')
        assert pair <= FP32_GRADE, pair
    full = eng.render(_c2w(), extras=True)
    assert set(full) == set(out)
    for k in out:
        assert torch.equal(_bits(full[k][:n]), _bits(out[k])), k
    eng.close()


# ---- c. the second exit and the coarse stream without its view branch, with given directions ---------------------------------------
@pytest.mark.parametrize('shape', ['n139', 's67'])
@pytest.mark.parametrize('mode', ['fp16x3_asm', 'fp16_mix'])
def test_skip_rgb0_with_given_directions_changes_no_map(pkg, frame, mode, shape):
    """nerf_set_skip_rgb0 on an NDC engine: every map and extra except rgb0 and raw bit for bit, every density of raw bit for bit, zero
    colours exactly on the fine launch's 128-point tiles without a positive density (the indexing of
    test_second_exit_behind_the_density_changes_no_map; the short last tile: zero if it has none, the full chain's otherwise)"""
    n = SHAPES[shape][0]
    eng = _engine(shape, mode, sds=_sparse())
    ro, rd = frame['ro'][:n].cuda(), frame['rd'][:n].cuda()
    full = {k: v.clone() for k, v in eng.render_rays(ro, rd, extras=True).items()}
    eng.set_skip_rgb0(True)
    got = eng.render_rays(ro, rd, extras=True)
    assert set(got) == set(full) - {'rgb0'}
    for k in got:
        if k != 'raw':
            assert torch.equal(_bits(got[k]), _bits(full[k])), k
    raw, raw_f = got['raw'].reshape(-1, 4), full['raw'].reshape(-1, 4)
    assert torch.equal(_bits(raw[:, 3]), _bits(raw_f[:, 3]))
    m = raw.shape[0] // 128 * 128
    assert m < raw.shape[0]                                                     # a short last tile: the shape is ragged
    dead = ~(raw_f[:m, 3] > 0).reshape(-1, 128).any(-1)
    share = float(dead.float().mean())
    print(f'{mode} {shape}: {share:.3f} of the fine launch\'s {dead.numel()} whole tiles have no positive density; acc_map up to {float(full["acc_map"].max()):.3f}')
    assert 0.2 <= share <= 0.9, share
    tiles, tiles_f = raw[:m, :3].reshape(-1, 128, 3), raw_f[:m, :3].reshape(-1, 128, 3)
    assert bool(tiles_f[dead].any())                                            # the full chain computed colours there
    assert not tiles[dead].any() and torch.equal(_bits(tiles[~dead]), _bits(tiles_f[~dead]))
    if bool((raw_f[m:, 3] > 0).any()):
        assert torch.equal(_bits(raw[m:, :3]), _bits(raw_f[m:, :3]))
    else:
        assert not raw[m:, :3].any()
    eng.set_skip_rgb0(False)
    again = eng.render_rays(ro, rd, extras=True)
    assert all(torch.equal(_bits(again[k]), _bits(full[k])) for k in full)
    eng.close()


# ---- d. `auto` on an NDC engine -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('limits,want', [({}, 'fp16x1'), (dict(max_diff_x1=0.0), 'fp16_fp8'), (dict(max_diff_x1=0.0, max_diff=0.0), 'fp16_mix'),
                                         (dict(max_diff_x1=0.0, max_diff=0.0, max_diff_mix=0.0), 'fp16x3_asm')])
def test_auto_precision_on_an_ndc_engine(pkg, frame, limits, want):
    """the ladder of test_teacher_auto_precision_is_measured on a forward-facing engine, probed with the world rays: fp16_mix and
    fp16x3_asm are reachable (their stage-by-stage check against fp16x3 re-evaluates the fine pass on the PROJECTED rays with the world
    rays' directions; on the caller's rays it compared unrelated points and ended on fp16x3), and the frame rendered afterwards is inside
    the contract"""
    from efficient_nerf_amd import PRECISIONS
    eng = _engine('frame')
    ro, rd = frame['ro'].cuda(), frame['rd'].cuda()
    name, diff = eng.choose_precision(ro, rd, **limits)
    print(f'limits {limits}: differences from fp16x3 {eng.auto_diffs} -> {name}; fp16x3_asm stage by stage: {eng.auto_detail.get("fp16x3_asm")}')
    if want in ('fp16_mix', 'fp16x3_asm'):
        assert eng.auto_diffs['fp16x3_asm'] <= eng.AUTO_MAX_DIFF_X3ASM and {'rgb0', 'acc0'} <= set(eng.auto_detail['fp16x3_asm'][0])
    assert name == want and eng.precision_name == want and eng.precision == PRECISIONS[want], (name, diff)
    err = (eng.render_rays(ro, rd)['rgb_map'].cpu() - _oracle(frame, 'frame')['rgb_map']).abs().max().item()
    print(f'   the frame in {name}: rgb_map {err:.2e} from the oracle')
    assert err <= 1e-4, err
    eng.close()


# ---- e. the watch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['fp16x1', 'fp16_fp8', 'fp16_mix', 'fp16x3_asm'])
def test_spot_check_on_an_ndc_engine(pkg, frame, mode):
    """spot_check of a frame an NDC engine rendered in a watched mode: ok, under the mode's limits, the mode kept; and the fp16x3_asm
    check is live (a zero limit fails it with finite, non-zero differences)"""
    eng = _engine('frame', mode)
    limit = {'fp16x1': eng.AUTO_MAX_DIFF_X1, 'fp16_fp8': eng.AUTO_MAX_DIFF, 'fp16_mix': eng.AUTO_MAX_DIFF_MIX, 'fp16x3_asm': eng.AUTO_MAX_DIFF_X3ASM}[mode]
    lim = eng._limits(limit)
    if mode == 'fp16x3_asm':
        lim['rgb0'] = lim['acc0'] = limit
    ro, rd = frame['ro'].cuda(), frame['rd'].cuda()
    got = eng.render_rays(ro, rd)
    ok, d = eng.spot_check(ro, rd, got)
    print(f'{mode}: spot check {ok}, {d} (limits {lim})')
    assert ok and set(lim) <= set(d) and all(d[k] <= lim[k] for k in lim), d
    assert eng.precision_name == mode
    if mode == 'fp16x3_asm':
        eng.AUTO_MAX_DIFF_X3ASM = 0.0
        ok0, d0 = eng.spot_check(ro, rd, got)
        print(f'   with a zero limit: {ok0}, {d0}')
        assert not ok0 and all(math.isfinite(v) for v in d0.values()) and max(d0[k] for k in lim) > 0
        assert eng.precision_name == mode
    eng.close()


def test_render_path_keeps_fp16x3_asm_on_an_ndc_engine(pkg, frame):
    """frontend.render_path over three nearby poses with the watch on every frame: an explicit fp16x3_asm is not stepped down on a
    forward-facing engine, and every frame is inside the contract against O.teacher_render(..., ndc=True)"""
    from efficient_nerf_amd import frontend as fe
    eng = _engine('frame', 'fp16x3_asm')
    poses = []
    for dx in (0., 0.02, -0.03):
        c = _c2w()
        c[0, 3] += dx
        poses.append(c)
    st = {}
    rgbs, _ = fe.render_path(poses, (H, W, FOCAL), 'nerf', eng, log=lambda *a: None, stats=st, watch_every=1)
    w = st['watch']
    print(w)
    assert w['checks'] == 3 and not w['fallbacks'] and w['precision'] == 'fp16x3_asm' and eng.precision_name == 'fp16x3_asm'
    t0, t1 = _plain()
    for i, c in enumerate(poses):
        ref = O.teacher_render(t0, t1, H, W, FOCAL, c, near=NEAR, far=FAR, ndc=True, white_bkgd=True)['rgb_map']
        err = (rgbs[i].reshape(-1, 3).cpu() - ref).abs().max().item()
        print(f'   frame {i}: rgb {err:.2e} from the oracle')
        assert err <= 1e-4, (i, err)
    eng.close()
