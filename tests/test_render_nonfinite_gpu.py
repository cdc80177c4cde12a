"""GPU: a non-finite ray through the fused R2L renderers.  The reference decides: for every ray the renderers give NaN
exactly where float32 torch on the CPU does (oracle.r2l_forward over positional_embed(sample_rays(...))), and every other ray of the
call keeps its bits.  The generated streams' v_max ReLU and r2l_act's fmaxf drop a NaN and render such a ray as a believable colour from
h0 = 0; the rule is enforced behind them, where it depends on the ray alone (r2l_mark_nonfinite_kernel; a host pose is checked on the host).

Every case takes its masks from the oracle and first asserts that they are the table's (tests/nonfinite_cases.py: RAY_POISONS,
STUDENT_NAN).  It then checks (1) the NaN masks element for element and no new infinity, (2) that every unpoisoned ray is int32-equal to
the same call with each poisoned ray replaced by a copy of its clean neighbour, (3) that the engine's state (activation exponents, range
status, guarded launches, mode) is the same after both calls -- a fresh engine per call, so that the calibration is open in both --, and
(4) that every slot of a sentinel-filled output was written and none behind it.  Clean rays are held to the oracle under the limits of
tests/test_r2l_gpu.py (1e-4 for the modes under the contract, 5e-3 for the single fp16 pass).

n = 300 given rays are three 128-ray tiles, the last ragged; the poisons sit on ray 0, on 31 | 32 (a wave and a lane half meet), on
127 | 128 (a tile edge) and on 299, which the head kernel repeats into the padding lanes.  Two rotations of the six poisons over the six
positions give every position a poison that is NaN in the reference (poison 4, rays_d = 0, is finite for the student)."""
import functools

import pytest
import torch

import nonfinite_cases as NC
from oracle import r2l_oracle as O

pytestmark = pytest.mark.gpu

N = 300
POSITIONS = (0, 31, 32, 127, 128, 299)
SHIFTS = (0, 3)
MODES = ('fp16x3', 'fp16x1', 'fp16_fp8', 'fp16_e4m3', 'fp16x3_asm', 'fp16_split', 'fp16_split8')
TWO_PART = ('fp16_split', 'fp16_split8')
TOL = {m: 1e-4 for m in MODES}
TOL['fp16x1'] = 5e-3
#: (n_block, mode, split block): W = 256; every mode at 0, 1 and 5 blocks, the two-part modes with split 0, 2 and 5 of 5; 43 blocks once
CASES = [(nb, m, sp) for nb in (0, 1, 5) for m in MODES for sp in ((0, 2, 5) if (m in TWO_PART and nb == 5) else (None,))] + [(43, 'fp16_fp8', None)]


@functools.lru_cache(None)
def _state(nb):
    return O.make_r2l_state(0, netdepth=2 + 2 * nb)


@functools.lru_cache(None)
def _rays(shift):
    ro, rd, _ = NC.frame_rays(15, 20)
    assert ro.shape[0] == N
    return NC.poisoned_pair(ro, rd, POSITIONS, shift)


@functools.lru_cache(None)
def _oracle(nb, shift, use_residual=True, act='relu'):
    """the oracle's rgb of the poisoned set in float32, checked against the table; computed once per network"""
    bo, bd, _, _, kinds = _rays(shift)
    with torch.no_grad():
        emb = O.positional_embed(O.sample_rays(bo, bd, O.sampler_z_vals(16, 2., 6.)), 10)
        ref = O.r2l_forward(_state(nb), emb, use_residual=use_residual, act=act, inact=act)
    nan = torch.isnan(ref)
    for r in range(N):
        want = NC.STUDENT_NAN[kinds[r]] if r in kinds else False
        assert bool(nan[r].all()) == want and bool(nan[r].any()) == want, (r, kinds.get(r), ref[r])     # all three channels or none
    assert not torch.isinf(ref).any()
    return ref


def _engine(nb, mode, split=None, **kw):
    from efficient_nerf_amd import PRECISIONS, R2LEngine
    eng = R2LEngine(12, 12, O.focal_from_angle(12), n_block=nb, precision=PRECISIONS[mode], **kw).load_state_dict(_state(nb))
    if split is not None:
        eng.set_split_block(split)
    return eng


def _snapshot(eng):
    """what a render may leave behind in the engine; the range status exists in the modes with operand scales (no clamp may be reported)"""
    from efficient_nerf_amd.r2l import SPLIT_MODES
    status = eng.range_status() if eng.precision in SPLIT_MODES and eng.n_block > 0 else None
    assert status is None or not status['saturated'], status
    return dict(exps=eng.act_exponents(), status=status, precision=eng.precision, split=eng.split_block)


def _render_pair(make, shift):
    """the poisoned set and the set with duplicates, each on an engine of its own: (rgb, whole buffer, state) x 2"""
    bo, bd, do, dd, _ = _rays(shift)
    res = []
    for ro, rd in ((bo, bd), (do, dd)):
        eng = make()
        out, whole = NC.sentinel_like((N, 3), 'cuda')
        eng.render_rays(ro.cuda(), rd.cuda(), out=out)
        torch.cuda.synchronize()
        res.append((out, whole, _snapshot(eng)))
        eng.close()
    return res


def _check_pair(res, ref, shift, tol, what):
    (got, whole, st), (dup, dwhole, dst) = res
    kinds = _rays(shift)[4]
    clean = NC.clean_mask(N, kinds)
    g = got.cpu()
    err = float((g - ref)[clean].abs().max())
    print(f'{what} shift {shift}: NaN rays {sorted(int(r) for r in torch.isnan(g).any(-1).nonzero().flatten())}, clean rays L_inf vs the oracle {err:.3e}')
    assert torch.equal(torch.isnan(g), torch.isnan(ref)), (what, 'NaN mask', torch.isnan(g).any(-1).nonzero().flatten().tolist())   # (1)
    assert NC.no_new_inf(g, ref), (what, 'an infinity the oracle does not have')
    assert NC.int32_equal(got, dup, clean.cuda()), (what, 'an unpoisoned ray changed its bits')                                     # (2)
    assert st == dst, (what, st, dst)                                                             # (3)
    assert NC.written_exactly(got, whole) and NC.written_exactly(dup, dwhole), (what, 'slots unwritten, or written behind the end')  # (4)
    assert err <= tol, (what, err)


@pytest.mark.parametrize('nb,mode,split', CASES, ids=[f'{nb}blk-{m}' + ('' if sp is None else f'-split{sp}') for nb, m, sp in CASES])
def test_given_rays_in_every_mode(pkg, nb, mode, split):
    """render_rays on the 300 rays, both rotations of the poisons: masks, neighbours' bits, engine state, written slots, clean values"""
    for shift in SHIFTS:
        _check_pair(_render_pair(lambda: _engine(nb, mode, split), shift), _oracle(nb, shift), shift, TOL[mode], f'{mode} n_block {nb} split {split}')


def test_the_generic_path_is_the_control(pkg):
    """GenericR2L.render_rays on the same rays: the fp32 layer path has followed torch on NaN since its ReLU was mended"""
    from efficient_nerf_amd.generic import GenericR2L
    for nb in (1, 5):
        for shift in SHIFTS:
            bo, bd, do, dd, kinds = _rays(shift)
            g = GenericR2L(12, 12, O.focal_from_angle(12), netdepth=2 + 2 * nb, netwidth=256, trial=dict(body_arch='resmlp')).load_state_dict(_state(nb))
            out, whole = NC.sentinel_like((N, 3), 'cuda')
            g.render_rays(bo.cuda(), bd.cuda(), out=out)
            dup = g.render_rays(do.cuda(), dd.cuda())
            ref, clean = _oracle(nb, shift), NC.clean_mask(N, kinds)
            assert torch.equal(torch.isnan(out.cpu()), torch.isnan(ref)) and NC.no_new_inf(out.cpu(), ref)
            assert NC.int32_equal(out, dup, clean.cuda()) and NC.written_exactly(out, whole)
            assert float((out.cpu() - ref)[clean].abs().max()) <= 1e-4


@pytest.mark.parametrize('mode', ['fp16_fp8', 'fp16_split'])
@pytest.mark.parametrize('fused', [True, False])
def test_fused_tail_on_and_off(pkg, mode, fused):
    """the body kernel's fused tail, and the three-launch form with r2l_tail_kernel behind it"""
    _check_pair(_render_pair(lambda: _engine(5, mode)._set_fused_tail(fused), 0), _oracle(5, 0), 0, TOL[mode], f'{mode} fused tail {fused}')


@pytest.mark.parametrize('mode', ['fp16x3', 'fp16_e4m3'])
def test_without_the_global_skip(pkg, mode):
    """use_residual = False: the generated modes finish the rays in r2l_tail_kernel on the body's output alone"""
    _check_pair(_render_pair(lambda: _engine(5, mode, use_residual=False), 3), _oracle(5, 3, use_residual=False), 3, TOL[mode], f'{mode} no skip')


@pytest.mark.parametrize('mode', ['fp16x3', 'fp16x1'])
def test_general_activation_build(pkg, mode):
    """LeakyReLU everywhere: the second instantiation of the compiler-scheduled kernel (max(v, 0.01 v) keeps a NaN; the ray is marked all the same)"""
    _check_pair(_render_pair(lambda: _engine(5, mode, act='lrelu', inact='lrelu'), 0), _oracle(5, 0, act='lrelu'), 0, TOL[mode], f'{mode} lrelu')


def _bad_poses():
    good = torch.as_tensor(O.pose_spherical(30., -30., 4.))[:3, :4].float().contiguous()
    nan_t, inf_r = good.clone(), good.clone()
    nan_t[1, 3] = NC.NAN
    inf_r[0, 1] = NC.INF
    return good, {'nan_translation': nan_t, 'inf_rotation': inf_r}


@pytest.mark.parametrize('mode', MODES)
def test_render_with_a_poisoned_host_pose(pkg, mode):
    """render(c2w) of an 8 x 8 frame with a NaN translation, and with an infinity in one rotation entry: the masks of oracle.r2l_render, every slot
    written; the same engine then renders a clean pose within the mode's limit, and a pose with finite entries large enough to overflow
    under 2^9 is not waved through by the host's check"""
    H = 8
    focal = O.focal_from_angle(H)
    from efficient_nerf_amd import PRECISIONS, R2LEngine
    eng = R2LEngine(H, H, focal, n_block=5, precision=PRECISIONS[mode]).load_state_dict(_state(5))
    good, bad = _bad_poses()
    huge = good.clone()
    huge[2, 3] = 3e38
    bad['huge_translation'] = huge
    for name, c2w in bad.items():
        ref = O.r2l_render(_state(5), H, H, focal, c2w)
        assert torch.isnan(ref).all(), name          # every ray of such a frame is poisoned
        out, whole = NC.sentinel_like((H * H, 3), 'cuda')
        eng.render(c2w, out=out)
        assert torch.equal(torch.isnan(out.cpu()), torch.isnan(ref)) and NC.written_exactly(out, whole), (mode, name)
    err = float((eng.render(good).cpu() - O.r2l_render(_state(5), H, H, focal, good)).abs().max())
    assert err <= TOL[mode], (mode, err)
    eng.close()


@pytest.mark.parametrize('mode', ['fp16x3', 'fp16_fp8', 'fp16x3_asm', 'fp16_split8'])
def test_render_batch_with_the_second_pose_poisoned(pkg, mode):
    """two device poses at 12 x 12: 144 rays per pose, so ray tile 1 holds rays of both.  Frame 0 is bit for bit its single render, frame 1 has
    the oracle's masks; with the second pose clean instead the engine ends in the same state"""
    H = 12
    focal = O.focal_from_angle(H)
    good, bad = _bad_poses()
    for name, c2w in bad.items():
        ref1 = O.r2l_render(_state(5), H, H, focal, c2w)
        eng = _engine(5, mode)
        out, whole = NC.sentinel_like((2, H * H, 3), 'cuda')
        eng.render_batch(torch.stack([good, c2w]).cuda(), out=out)
        st = _snapshot(eng)
        eng.close()
        single = _engine(5, mode)
        one = single.render_batch(good[None].cuda())
        single.close()
        dup = _engine(5, mode)
        two = dup.render_batch(torch.stack([good, good]).cuda())
        dst = _snapshot(dup)
        dup.close()
        assert NC.int32_equal(out[0], one[0]) and NC.int32_equal(out[0], two[0]), (mode, name, 'frame 0 changed its bits')
        assert torch.equal(torch.isnan(out[1].cpu()), torch.isnan(ref1)) and NC.no_new_inf(out[1].cpu(), ref1), (mode, name)
        assert NC.written_exactly(out, whole)
        assert st == dst, (mode, name, st, dst)
        assert float((out[0].cpu() - O.r2l_render(_state(5), H, H, focal, good)).abs().max()) <= TOL[mode]


def test_sample_embed_of_a_poisoned_pose(pkg):
    """the stand-alone sampler + embedder: points bit for bit the oracle's (NaN where it has NaN), NaN in exactly the oracle's columns of the
    embedding -- the 20 sin / cos columns of every poisoned coordinate --, and the identity column carries the point's own bits"""
    from efficient_nerf_amd import R2LEngine
    H = 8
    focal = O.focal_from_angle(H)
    eng = R2LEngine(H, H, focal, n_block=0)
    good, bad = _bad_poses()
    huge = good.clone()
    huge[0, 3] = 3e38                      # finite points; x 2^l overflows from l = 1 on
    bad['huge_translation'] = huge
    z = O.sampler_z_vals(16, 2., 6.)
    for name, c2w in bad.items():
        pts_ref = O.sample_test(O.camera_dirs(H, H, focal), z, c2w)
        emb_ref = O.positional_embed(pts_ref, 10)
        pts, emb = eng.sample_embed(c2w)
        assert NC.same_bits(pts.cpu(), pts_ref), name
        assert torch.equal(torch.isnan(emb.cpu()), torch.isnan(emb_ref)), name
        assert torch.equal(torch.isinf(emb.cpu()), torch.isinf(emb_ref)), name
        e = emb.view(H * H, 48, 21)
        assert NC.int32_equal(e[:, :, 20], pts), name
        bad_cols = torch.isnan(emb_ref).view(H * H, 48, 21)[:, :, :20]
        assert bool((bad_cols.all(-1) | ~bad_cols.any(-1)).all()) or name == 'huge_translation'     # a poisoned coordinate: all 20, else none
        # values: the coordinates the poison left alone (sin(3e38) is a number on both sides, but what it is worth at that magnitude is the
        # huge-finite question DESIGN.md §4 leaves to the range guard)
        sound = torch.isfinite(emb_ref).view(H * H, 48, 21).all(-1)
        assert float((emb.cpu() - emb_ref).view(H * H, 48, 21)[sound].abs().max()) <= 5e-7, name
    eng.close()


@pytest.mark.parametrize('L', [10, 4])
def test_positional_embedder_on_a_tensor(pkg, L):
    """PositionalEmbedder on a device tensor with NaN (with a payload), +-Inf and 3e38 among its entries: NaN in exactly the oracle's columns
    of that entry's 2 L + 1 (3e38: from the octave at which x 2^l overflows), the identity column the input's own bits, the rest within 5e-7"""
    from efficient_nerf_amd import PositionalEmbedder
    x = torch.randn(301, 6, generator=torch.Generator().manual_seed(7)) * 3
    x[0, 0], x[17, 5], x[300, 2], x[128, 3] = NC.NAN, NC.INF, -NC.INF, 3e38
    xi = x.view(torch.int32)
    xi[64, 1] = 0x7FC12345
    xi[65, 4] = -4194304 + 0x777           # 0xFFC00777: a negative NaN with a payload
    ref = O.positional_embed(x, L)
    got = PositionalEmbedder(L)(x.cuda())
    assert torch.equal(torch.isnan(got.cpu()), torch.isnan(ref)) and torch.equal(torch.isinf(got.cpu()), torch.isinf(ref))
    assert int(torch.isnan(ref).view(301, 6, 2 * L + 1)[:, :, :2 * L].all(-1).sum()) == 5 and bool(torch.isnan(ref).view(301, 6, 2 * L + 1)[128, 3, 1:L].all())
    assert NC.int32_equal(got.view(301, 6, 2 * L + 1)[:, :, 2 * L], x.cuda())
    sound = torch.isfinite(ref).view(301, 6, 2 * L + 1).all(-1)          # the entries without a poison (sin(3e38) itself: see above)
    assert int((~sound).sum()) == 6 and float((got.cpu() - ref).view(301, 6, 2 * L + 1)[sound].abs().max()) <= 5e-7


def test_fp16_fp8_render_in_a_captured_graph(pkg):
    """one fp16_fp8 render of the 300 rays inside a captured graph, replayed once on the poisoned set: the marking pass is stream-ordered
    device work like the rest of the call"""
    bo, bd, do, dd, kinds = _rays(0)
    eng = _engine(5, 'fp16_fp8')
    so, sdir = do.cuda().clone(), dd.cuda().clone()
    out = torch.empty((N, 3), device='cuda')
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):                # warm-up on the capture stream, on the clean set: buffers allocated, exponents measured
        for _ in range(2):
            eng.render_rays(so, sdir, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        eng.render_rays(so, sdir, out=out)
    so.copy_(bo)
    sdir.copy_(bd)
    out.view(torch.int32).fill_(NC.SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    ref = _oracle(5, 0)
    direct = eng.render_rays(bo.cuda(), bd.cuda())
    assert NC.int32_equal(out, direct)
    assert torch.equal(torch.isnan(out.cpu()), torch.isnan(ref)) and bool((out.view(torch.int32) != NC.SENTINEL).all())
    assert float((out.cpu() - ref)[NC.clean_mask(N, kinds)].abs().max()) <= TOL['fp16_fp8']
    eng.close()


def test_choose_precision_ends_on_the_same_rung(pkg):
    """`auto` on the poisoned set and on the set with duplicates: the same mode, the same exponents, the same largest |activation|; its
    verification against three passes compares the rays that are numbers on both sides (r2l.watch_diff)"""
    bo, bd, do, dd, kinds = _rays(0)
    res = []
    for ro, rd in ((bo, bd), (do, dd)):
        eng = _engine(5, 'fp16x3')
        name, top = eng.choose_precision(rays=(ro.cuda(), rd.cuda()))
        res.append((name, top, eng.stream_max, eng.split_block, eng.act_exponents(), eng.auto_verify))
        eng.close()
    print('auto on the poisoned set / with duplicates:', res)
    assert res[0][:5] == res[1][:5] and res[0][5] <= eng.AUTO_VERIFY_MAX_DIFF and res[1][5] <= eng.AUTO_VERIFY_MAX_DIFF


# ---------------------------------------------------------------------------------------------------------------------------------
# the watches: poisoned rays at the strided indices they sample
# ---------------------------------------------------------------------------------------------------------------------------------
WATCH_RAYS = 100                                  # of 300: every third ray (R2LEngine._strided_rays)
WATCH_POS = (0, 33, 126, 129, 297, 150)           # all multiples of three


def _watch_rays():
    ro, rd, _ = NC.frame_rays(15, 20)
    return NC.poisoned_pair(ro, rd, WATCH_POS, 0)


def _sampled(eng, ro, rd):
    so, sd = eng._strided_rays(ro, rd, WATCH_RAYS)
    assert so.shape[0] == WATCH_RAYS
    return so, sd


@pytest.mark.parametrize('mode', ['fp16_fp8', 'fp16_e4m3', 'fp16_split', 'fp16_split8'])
def test_rgb_watch_with_poisoned_rays_among_the_sampled(pkg, mode, monkeypatch):
    """spot_check_rgb (fp16_fp8 / fp16_e4m3: against the three-pass watch context) and spot_check_split (the split in use against three passes
    everywhere): both renders give the same NaN mask, so the watch passes, reports the largest difference over the other elements and leaves
    the mode alone; with the mask of one side altered -- a NaN ray rendered finite, or a clean ray NaN -- it fails"""
    from efficient_nerf_amd import R2LEngine
    bo, bd, _, _, kinds = _watch_rays()
    bo, bd = bo.cuda(), bd.cuda()
    eng = _engine(5, mode, 2 if mode in TWO_PART else None)
    so, sd = _sampled(eng, bo, bd)
    sampled_nan = torch.isnan(eng.render_rays(so, sd)).all(-1)
    assert int(sampled_nan.sum()) == 5            # the five NaN poisons; rays_d = 0 is finite
    before = (eng.precision, eng.split_block)
    ok, d = eng.spot_check_rgb(bo, bd, n_rays=WATCH_RAYS)
    # what it must have compared: this mode against three passes on the sampled rays that are numbers
    got = eng.render_rays(so, sd).clone()
    if mode in TWO_PART:
        eng.set_split_block(5)
        ref = eng.render_rays(so, sd).clone()
        eng.set_split_block(2)
    else:
        ref = eng._watch_engine().render_rays(so, sd).clone()
    want = float((got - ref)[~sampled_nan].abs().max())
    limit = eng.SPLIT_WATCH_MAX_DIFF if mode in TWO_PART else eng.WHOLE_WATCH_MAX_DIFF
    print(f'{mode}: watch ok {ok}, difference {d:.3e} (by hand {want:.3e}, limit {limit:g})')
    assert ok and d == want and 0 < d <= limit and (eng.precision, eng.split_block) == before
    assert torch.equal(torch.isnan(got), torch.isnan(ref))

    # one side's mask altered: the reference render gives a number for the first NaN ray / a NaN for a clean ray
    target = eng if mode in TWO_PART else eng._watch_engine()
    real = R2LEngine.render_rays
    first_nan, first_clean = int(sampled_nan.nonzero()[0]), int((~sampled_nan).nonzero()[0])
    for row, value in ((first_nan, 0.5), (first_clean, NC.NAN)):
        calls = []

        def altered(self, rays_o, rays_d, out=None, _row=row, _value=value):
            rgb = real(self, rays_o, rays_d, out)
            calls.append(self)
            # the reference side: the watch context, or this context's second render (three passes everywhere)
            if self is target and (mode not in TWO_PART or len([c for c in calls if c is target]) == 2):
                rgb[_row, 1] = _value
            return rgb

        monkeypatch.setattr(R2LEngine, 'render_rays', altered)
        ok, d = eng.spot_check_rgb(bo, bd, n_rays=WATCH_RAYS)
        monkeypatch.setattr(R2LEngine, 'render_rays', real)
        assert not ok and d != d, (mode, row, value, ok, d)
    eng.close()


def test_rgb_watch_on_an_all_nan_sample(pkg, capsys):
    """every sampled ray poisoned: nothing to compare -- a pass with difference 0, counted and said"""
    ro, rd, _ = NC.frame_rays(15, 20)
    ro[::3, 0] = NC.NAN
    eng = _engine(5, 'fp16_fp8')
    ok, d = eng.spot_check_rgb(ro.cuda(), rd.cuda(), n_rays=WATCH_RAYS)
    assert ok and d == 0.0 and eng.watch_all_nan == 1
    assert 'NaN in both renders' in capsys.readouterr().err
    eng.close()
