"""GPU: frontend.render_path's teacher watch on the shared loop (efficient-nerf_amd/watch.py) with a real NeRFEngine whose spot_check is
replaced by a stub that misses a given number of times, and render_path's picture side (_PictureSink) with and without --png_device.
8 x 8 and 16 x 16 frames: what is under test is the loop around the renders."""
import os

import numpy as np
import pytest
import torch

from oracle import r2l_oracle as O

pytestmark = pytest.mark.gpu
LADDER = ('fp16x1', 'fp16_fp8', 'fp16_mix', 'fp16x3_asm', 'fp16x3')


def _watched_path(misses):
    """three 8 x 8 frames, watch_every = 1, from fp16x1, the first `misses` spot checks fail; returns (frames, stats, the '[precision]
    frame' lines, how often each pose was rendered, the same frames rendered plainly in the mode the engine ended in)"""
    from efficient_nerf_amd import NeRFEngine, PRECISIONS, frontend as fe
    H = 8
    focal = O.focal_from_angle(H)
    sds = (O.make_teacher_state(3), O.make_teacher_state(4))
    poses = [O.pose_spherical(th, -30., 4.) for th in (-60., 20., 100.)]
    eng = NeRFEngine(H, H, focal, N_samples=16, N_importance=32, precision=PRECISIONS['fp16x1']).load_state_dicts(*sds)
    checks, renders = [], []

    def spot_check(ro, rd, got):
        checks.append(eng.precision_name)
        return len(checks) > misses, {'rgb_map': 1.0}

    render = eng.render
    eng.spot_check = spot_check
    eng.render = lambda pose, **kw: renders.append(next(k for k, p in enumerate(poses) if torch.equal(p[:3, :4], pose))) or render(pose, **kw)
    st, lines = {}, []
    rgbs, _ = fe.render_path(poses, (H, H, focal), 'nerf', eng, log=lines.append, stats=st, watch_every=1)
    rgbs = rgbs.cpu()
    ended = eng.precision_name
    eng.close()
    ref = NeRFEngine(H, H, focal, N_samples=16, N_importance=32, precision=PRECISIONS[ended]).load_state_dicts(*sds)
    ref.set_skip_rgb0(True)                                    # as render_path sets it: rgb only
    plain = torch.stack([ref.render(p[:3, :4])['rgb_map'].reshape(H, H, 3).cpu() for p in poses], 0)
    ref.close()
    return rgbs, st, [ln for ln in lines if ln.startswith('[precision] frame')], renders, plain, checks


def _line(i, was, now):
    return (f"[precision] frame {i}: {was} is {{'rgb_map': 1.0}} from fp16x3 on 2048 of its rays (limits {'3e-05' if was == 'fp16x1' else '2e-05'} x (1, 1, far)) "
            f"-> {now}; frame rendered again")


def test_four_misses_on_a_frame_walk_the_whole_ladder(pkg):
    """The case render_path got wrong while its teacher watch tried three times whatever the ladder's length: after misses in fp16x1,
    fp16_fp8 and fp16_mix the frame was rendered in fp16x3_asm and handed on unchecked.  Bounded by the ladder, the fourth miss is
    checked (and here forced), and the frame ends in fp16x3, where nothing is left to check."""
    rgbs, st, lines, renders, plain, checks = _watched_path(4)
    assert [(f['frame'], f['from'], f['to']) for f in st['watch']['fallbacks']] == [(0, LADDER[k], LADDER[k + 1]) for k in range(4)]
    assert st['watch'] == {'checks': 4, 'fallbacks': [{'frame': 0, 'from': LADDER[k], 'to': LADDER[k + 1], 'diffs': {'rgb_map': 1.0}} for k in range(4)],
                           'worst': {'rgb_map': 1.0}, 'every': 1, 'precision': 'fp16x3'}
    assert checks == list(LADDER[:4])                          # fp16x3_asm was checked; fp16x3 has nothing to compare with
    assert renders == [0] * 5 + [1, 2]                         # frame 0 once per rung, frames 1 and 2 once each
    assert lines == [_line(0, LADDER[k], LADDER[k + 1]) for k in range(4)]
    assert torch.equal(rgbs, plain)                            # frame 0 is a plain fp16x3 render bit for bit (and so are the two behind it)


def test_one_miss_steps_down_once_and_keeps_watching(pkg):
    """one forced miss: the records and the line as the loop written out in render_path produced them"""
    rgbs, st, lines, renders, plain, checks = _watched_path(1)
    assert st['watch'] == {'checks': 4, 'fallbacks': [{'frame': 0, 'from': 'fp16x1', 'to': 'fp16_fp8', 'diffs': {'rgb_map': 1.0}}],
                           'worst': {'rgb_map': 1.0}, 'every': 1, 'precision': 'fp16_fp8'}
    assert checks == ['fp16x1', 'fp16_fp8', 'fp16_fp8', 'fp16_fp8'] and renders == [0, 0, 1, 2]
    assert lines == [_line(0, 'fp16x1', 'fp16_fp8')]
    assert torch.equal(rgbs, plain)


def test_pictures_of_a_path_with_and_without_the_device_encoder(pkg, tmp_path, monkeypatch):
    """five 16 x 16 frames in batches of two with ground truth: `<i>.png` and `<i>_gt.png` for every frame, on the host path the bytes
    of write_png(to8b(.)) of stats['host_frames'] and of the ground truth, under png_device the encoder's own bytes for the same stacks
    (collected over two batches, then the short last one), and host_frames the rendered stack bit for bit either way"""
    from efficient_nerf_amd import PREC_FP16X3, R2LEngine, frontend as fe
    from efficient_nerf_amd.png import encode_png
    monkeypatch.setattr(fe, 'PNG_FRAMES_PER_CALL', 4)
    H, n = 16, 5
    focal = O.focal_from_angle(H)
    eng = R2LEngine(H, H, focal, n_block=3, precision=PREC_FP16X3).load_state_dict(O.make_r2l_state(seed=0, netdepth=8))
    poses = [O.pose_spherical(-180. + 47. * k, -30. + 5. * (k % 3), 4.) for k in range(n)]
    gt = torch.rand((n, H, H, 3), generator=torch.Generator().manual_seed(5))
    names = sorted(f'{i:03d}{tag}.png' for i in range(n) for tag in ('', '_gt'))
    host = {}
    for tag, dev in (('plain', False), ('device', True)):
        d, st = tmp_path / tag, {}
        os.makedirs(d)
        rgbs, misc = fe.render_path(poses, (H, H, focal), 'R2L', eng, gt_imgs=gt, savedir=str(d), log=lambda *a: None, stats=st,
                                    frames_per_batch=2, png_device=dev)
        assert sorted(os.listdir(d)) == names
        host[tag] = st['host_frames']
        assert torch.equal(host[tag], rgbs.cpu()) and not host[tag].is_cuda and 'test_psnr' in misc
        if dev:
            want = dict(zip(names[0::2], encode_png(rgbs)))
            want.update(zip(names[1::2], encode_png(gt.cuda())))
        else:
            for i in range(n):
                fe.write_png(str(tmp_path / names[2 * i]), fe.to8b(host[tag][i].numpy()))
                fe.write_png(str(tmp_path / names[2 * i + 1]), fe.to8b(gt[i].numpy()))
            want = {f: open(tmp_path / f, 'rb').read() for f in names}
        for f in names:
            assert open(d / f, 'rb').read() == want[f], (tag, f)
    assert torch.equal(host['plain'], host['device'])
    assert np.ptp(host['plain'].numpy()) > 0
    eng.close()
